"""Inputs and a plain reference model for csrc/thin_kernels.hip, the ordered medial-axis thinning (numpy / scipy / oracle.morph only,
never the code under test).

The model restates the kernel's dependency-DAG wavefront from the mask alone: the 64-bit order key of every pixel, its predecessor
byte, its level in the DAG (= the Jacobi round in which it is finished), the number of ma_round_kernel launches that follows from
the depth, and which 64 x 64 tiles go to sleep and have to wake.  tests/test_medial_cases.py holds the model against
oracle.morph.medial_axis and pins the properties of the inputs; tests/test_gpu_medial_stages.py holds the device against both."""
from __future__ import annotations

import numpy as np
from scipy import ndimage as ndi

import morph_cases as mc
from oracle import morph

MA_T, MA_R, MA_GROUP = 64, 16, 4          # tile side, halo = Jacobi rounds per launch, launches between two looks at the flags
BACKGROUND_KEY = np.uint64(2 ** 64 - 1)
EIGHT = np.ones((3, 3), bool)
# the 8 neighbours in raster order of the 3 x 3 window without its centre: bit k of a predecessor byte is neighbour k
NEIGHBOURS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
def framed(N):
    """the whole N x N frame minus a 1-px border"""
    m = np.zeros((N, N), bool)
    m[1:-1, 1:-1] = True
    return m


def wake_cases():
    """solid masks with long chains: tiles in the middle sleep while the front is far away and must wake when it arrives"""
    return [("full320", mc.full(320, 320)), ("full250x245", mc.full(250, 245)), ("framed386", framed(386)),
            ("disc220", np.ascontiguousarray(mc.disc(449, 449, 220))), ("triangle450", np.ascontiguousarray(mc.triangle(450, 450, 450)))]


SMALL_SHAPES = [s for s in mc.SHAPES if s != (513, 513)]
CHUNKS_SHAPE = (1030, 1021)               # 1027 chunks of 1024 pixels: ma_chunk_scan_kernel's slab loop takes a second trip


def chunks_mask():
    """sparse noise, runs across every multiple of 64 of the flat index, and blobs in the rows whose chunks lie beyond the 1024th, so
    that ranks from the scan's second slab decide ties between neighbours there"""
    H, W = CHUNKS_SHAPE
    m = mc.noise(H, W, 0.03, 4) | mc.runs64(H, W)
    m[1000:1028, 30:990] |= mc.blobs(28, 960, 5)
    return np.ascontiguousarray(m)


def chunks_batch():
    """the mask and its vertical flip: the second image starts at a pixel offset that is no multiple of 1024"""
    m = chunks_mask()
    return [("chunks", m), ("chunks_flipped", np.ascontiguousarray(m[::-1]))]


def mixed_batch():
    """depths from 0 to 1276 in one call: the shallow images are copied through for 70 launches after they have finished"""
    return [("empty", np.zeros((320, 320), bool)), ("full", mc.full(320, 320)), ("blobs", mc.blobs(320, 320)),
            ("noise45", mc.noise(320, 320, 0.45, 2)), ("framed", framed(320))]


# ------------------------------------------------------------------------------------------------------------------------------
# reference model
# ------------------------------------------------------------------------------------------------------------------------------
def ref_keys(mask):
    """(keys (H, W) u64, dist (H, W) f64): key = rint(dist^2) << 36 | (9 - c) << 32 | tie[rank]; background: 2^64 - 1"""
    m = np.asarray(mask, bool)
    dist = ndi.distance_transform_edt(m)
    c = ndi.correlate(m.astype(np.int64), np.ones((3, 3), np.int64), mode="constant", cval=0)
    nfg = int(m.sum())
    tie = np.random.RandomState(0).permutation(nfg).astype(np.uint64)          # indexed by the raster-order rank
    keys = np.full(m.shape, BACKGROUND_KEY, np.uint64)
    d2 = np.rint(dist[m] * dist[m]).astype(np.uint64)
    keys[m] = (d2 << np.uint64(36)) | ((9 - c[m]).astype(np.uint64) << np.uint64(32)) | tie
    return keys, dist


def ref_dep(keys):
    """(H, W) u8: bit k set when neighbour k is inside the frame and has a smaller key; 0 on the background"""
    H, W = keys.shape
    P = np.full((H + 2, W + 2), BACKGROUND_KEY, np.uint64)
    P[1:-1, 1:-1] = keys
    dep = np.zeros((H, W), np.uint8)
    for k, (dy, dx) in enumerate(NEIGHBOURS):
        dep |= (P[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] < keys).astype(np.uint8) << k
    dep[keys == BACKGROUND_KEY] = 0
    return dep


def ref_levels(dep, mask):
    """(H, W) i32: 1 for a foreground pixel without predecessors, else 1 + the largest level of its predecessors; 0 on the
    background.  Peeled front by front: a finished pixel takes one off the pending count of each successor."""
    m = np.asarray(mask, bool)
    H, W = m.shape
    Wp = W + 2
    depp = np.pad(dep, 1).ravel()
    pend = np.unpackbits(depp[:, None], axis=1).sum(axis=1).astype(np.int32)
    level = np.zeros((H + 2) * Wp, np.int32)
    front = np.flatnonzero(np.pad(m, 1).ravel() & (pend == 0))
    L = 0
    while front.size:
        L += 1
        level[front] = L
        succ = []
        for k, (dy, dx) in enumerate(NEIGHBOURS):
            s = front + (dy * Wp + dx)                           # the front pixel is neighbour 7 - k of its neighbour k
            succ.append(s[(depp[s] >> (7 - k)) & 1 == 1])
        s = np.concatenate(succ)
        np.subtract.at(pend, s, 1)
        u = np.unique(s)
        front = u[pend[u] == 0]
    level = level.reshape(H + 2, Wp)[1:-1, 1:-1]
    assert (level[m] > 0).all() and not level[~m].any()          # keys are distinct: the predecessor relation has no cycle
    return np.ascontiguousarray(level)


def skeleton_by_levels(mask, level):
    """the 512-entry table applied level by level, all pixels of a level at once on the running state (two pixels of one level are
    never neighbours): what the wavefront computes"""
    table = morph.medial_axis_table()
    m = np.asarray(mask, bool)
    H, W = m.shape
    Wp = W + 2
    res = np.pad(m.astype(np.int64), 1).ravel()
    idx = (np.arange(H)[:, None] + 1) * Wp + np.arange(W)[None, :] + 1
    flat, lv = idx[m], level[m]
    order = np.argsort(lv, kind="stable")
    flat, lv = flat[order], lv[order]
    bounds = np.searchsorted(lv, np.arange(1, (int(lv.max()) if lv.size else 0) + 2))
    wts = (1, 2, 4, 8, 32, 64, 128, 256)
    for a, b in zip(bounds[:-1], bounds[1:]):
        p = flat[a:b]
        acc = np.full(p.shape, 16, np.int64)
        for w, (dy, dx) in zip(wts, NEIGHBOURS):
            acc += w * res[p + (dy * Wp + dx)]
        res[p] = table[acc]
    return res.reshape(H + 2, Wp)[1:-1, 1:-1].astype(bool)


def expected_launches(depth):
    """ma_round_kernel launches of a call whose deepest image has `depth` levels: a launch finishes the next MA_R levels, the flags
    are read every MA_GROUP launches"""
    per_group = MA_GROUP * MA_R
    return MA_GROUP * max(1, -(-int(depth) // per_group))


_MODELS = {}


def model(key, mask):
    """dict(skel, dist, keys, dep, level, depth) of one mask, computed once per process under `key`; skel and dist are
    oracle.morph.medial_axis's"""
    if key not in _MODELS:
        m = np.ascontiguousarray(mask, bool)
        keys, dist = ref_keys(m)
        dep = ref_dep(keys)
        level = ref_levels(dep, m)
        skel, odist = morph.medial_axis(m)
        assert np.array_equal(dist, odist)
        r = dict(mask=m, skel=skel, dist=dist, keys=keys, dep=dep, level=level, depth=int(level.max()) if level.size else 0)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _MODELS[key] = r
    return _MODELS[key]


# ------------------------------------------------------------------------------------------------------------------------------
# sleeping tiles
# ------------------------------------------------------------------------------------------------------------------------------
def tile_trace(level):
    """(progress, own): two (launches, tiles_y, tiles_x) bool arrays.  own[L]: a pixel of the tile's own MA_T x MA_T has its level in
    (MA_R L, MA_R L + MA_R], i.e. is finished by launch L; progress[L]: such a pixel lies in the tile's staged area minus its rim,
    rows MA_T j - (MA_R - 1) ... MA_T j + MA_T + MA_R - 2 and the matching columns, clipped to the frame.
    This bounds the kernel's flag from above and does not reproduce it: ma_round_kernel records progress only when a staged pixel
    really became done in that workgroup, and a halo pixel whose chain of this launch leaves the staged area does not finish there
    although its level lies in the launch's range.  So the tiles asleep in this model are a subset of those the kernel lets sleep, and
    woken_tiles' claim is weaker than the kernel's premise; an oversleeping tile of the kernel shows on the GPU, in the exact launch
    count and the skeleton."""
    H, W = level.shape
    ty, tx = -(-H // MA_T), -(-W // MA_T)
    n = max(1, -(-int(level.max()) // MA_R))
    ys, xs = np.nonzero(level)
    L = (level[ys, xs] - 1) // MA_R
    own = np.zeros((n, ty, tx), bool)
    prog = np.zeros((n, ty, tx), bool)
    own[L, ys // MA_T, xs // MA_T] = True
    reach = MA_R - 1
    for jy in ((ys - reach) // MA_T, (ys + reach) // MA_T):
        for jx in ((xs - reach) // MA_T, (xs + reach) // MA_T):
            prog[L, np.clip(jy, 0, ty - 1), np.clip(jx, 0, tx - 1)] = True
    return prog, own


def asleep_tiles(progress):
    """(launches, tiles_y, tiles_x) bool: asleep in launch L >= 1 = no tile of the 3 x 3 tile neighbourhood had progress in L - 1
    (a lower bound of the kernel's sleeping set, see tile_trace)"""
    asleep = np.zeros_like(progress)
    for L in range(1, len(progress)):
        asleep[L] = ~ndi.binary_dilation(progress[L - 1], EIGHT)
    return asleep


def woken_tiles(level):
    """(tiles_y, tiles_x) bool: tiles that were asleep in some launch and finish a pixel of their own in a later one.  Also asserts
    the kernel's design claim: a tile asleep in launch L finishes no pixel of its own in L."""
    progress, own = tile_trace(level)
    asleep = asleep_tiles(progress)
    assert not (asleep & own).any()
    slept = np.zeros(progress.shape[1:], bool)
    woken = np.zeros(progress.shape[1:], bool)
    for L in range(len(progress)):
        woken |= slept & own[L]
        slept |= asleep[L]
    return woken
