"""Inputs and plain references for the stages of csrc/morph_kernels.hip (numpy / scipy only, no GPU).

Inputs: binary masks that stress one mechanism of the kernels each -- the 64-lane run initialisation and the chunk-boundary union
of the labelling, the ballots of the per-label statistics inside a grid-stride loop, the sleeping tiles of the Zhang thinning.
References: component roots, per-root area / perimeter code counts, and the thinning's launch-by-launch trace, all from scipy.ndimage
and oracle/morph.py, never from the code under test."""
from __future__ import annotations

import numpy as np
from scipy import ndimage as ndi

from oracle import morph

EIGHT = np.ones((3, 3), bool)
ZH_IT, ZH_TI = 4, 48          # full iterations per thinning launch, inner tile side (csrc/morph_kernels.hip)


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
def stair(N):
    """one-pixel 4-connected `\\` staircase: with scikit-image's table it burns from its two ends, one step per full iteration"""
    y, x = np.mgrid[:N, :N]
    return (y == x) | (y == x + 1)


def full(H, W):
    return np.ones((H, W), bool)


def disc(H, W, r=None):
    """a disc in the middle of the frame, radius r (default: the largest that fits, at most 40)"""
    if r is None:
        r = min(40, (min(H, W) - 1) // 2)
    y, x = np.mgrid[:H, :W]
    return (y - H // 2) ** 2 + (x - W // 2) ** 2 <= r * r


def triangle(H, W, side=None):
    """the lower-left right triangle x <= y of a square of `side` (default: the largest that fits, at most 64)"""
    if side is None:
        side = min(H, W, 64)
    y, x = np.mgrid[:H, :W]
    return (x <= y) & (y < side)


def spiral(H, W):
    """rectangular spiral from (0, 0) inward: 1-px arms, one row / column of background between turns"""
    m = np.zeros((H, W), bool)
    steps = ((0, 1), (1, 0), (0, -1), (-1, 0))
    y = x = d = 0
    m[0, 0] = True

    def can(d):
        dy, dx = steps[d]
        y1, x1, y2, x2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if not (0 <= y1 < H and 0 <= x1 < W) or m[y1, x1]:
            return False
        return not (0 <= y2 < H and 0 <= x2 < W and m[y2, x2])

    while True:
        if not can(d):
            d = (d + 1) % 4
            if not can(d):
                return m
        y, x = y + steps[d][0], x + steps[d][1]
        m[y, x] = True


def serpentine(H, W):
    """1-px rows on every other line, joined at alternating ends"""
    m = np.zeros((H, W), bool)
    m[0::2] = True
    m[1::4, W - 1] = True
    m[3::4, 0] = True
    return m


def comb(H, W):
    """a spine along the top row with 1-px teeth on every other column"""
    m = np.zeros((H, W), bool)
    m[0] = True
    m[:, 0::2] = True
    return m


def checker(H, W):
    """single-pixel checkerboard: one 8-component held together by the NW / NE unions alone"""
    y, x = np.mgrid[:H, :W]
    return ((y + x) & 1).astype(bool)


def lattice(H, W):
    """isolated pixels: as many components as the frame can hold"""
    y, x = np.mgrid[:H, :W]
    return (y % 2 == 0) & (x % 2 == 0)


def runs64(H, W):
    """horizontal runs of 2..6 pixels across every multiple of 64 of the flat index (the labelling's chunk boundary), whatever the
    row they fall in"""
    f = np.zeros(H * W, bool)
    for k in range(64, H * W, 64):
        j = k // 64
        f[max(k - 1 - j % 3, 0):k + 1 + j % 4] = True
    return f.reshape(H, W)


def _two_discs(H, W, gap):
    """two discs stacked along the longer axis: the lower pole of the first and the upper pole of the second are single pixels;
    gap 1: the poles in one column with one background pixel between them; gap 0: the poles diagonal neighbours"""
    L, S = max(H, W), min(H, W)
    r = max(0, min((L - 4) // 4, (S - 2) // 2, 30))
    m = np.zeros((max(L, 4 * r + 4), max(S, 2 * r + 2)), bool)
    y, x = np.mgrid[:m.shape[0], :m.shape[1]]
    m |= (y - r) ** 2 + (x - r) ** 2 <= r * r
    cy, cx = (3 * r + 2, r) if gap else (3 * r + 1, r + 1)
    m |= (y - cy) ** 2 + (x - cx) ** 2 <= r * r
    m = m[:L, :S]
    return np.ascontiguousarray(m if H >= W else m.T)


def discs_gap(H, W):
    return _two_discs(H, W, 1)


def discs_diag(H, W):
    return _two_discs(H, W, 0)


def noise(H, W, p, seed=0):
    return np.random.RandomState(seed).uniform(size=(H, W)) < p


def blobs(H, W, seed=3):
    """smooth blobs like a segmentation of vessels (what the filter is made for)"""
    return ndi.gaussian_filter(np.random.RandomState(seed).normal(size=(H, W)), 3.0, mode="nearest") > 0.02


def cases(H, W):
    """[(name, mask)]: every generator at one frame size.  `full` is the whole frame (at 513 x 513: 65 removing launches, most tiles
    sleep and wake); the other solid shapes stay small here (stair and triangle <= 64, disc radius <= 40, disc pairs <= 30):
    solid_cases() has them at the sizes that matter for the thinning."""
    n = min(H, W, 64)
    st = np.zeros((H, W), bool)
    st[:n, :n] = stair(n)
    out = [("stair", st), ("full", full(H, W)), ("disc", disc(H, W)), ("triangle", triangle(H, W)), ("spiral", spiral(H, W)),
           ("serpentine", serpentine(H, W)), ("comb", comb(H, W)), ("checker", checker(H, W)), ("lattice", lattice(H, W)),
           ("runs64", runs64(H, W)), ("discs_gap", discs_gap(H, W)), ("discs_diag", discs_diag(H, W)),
           ("noise35", noise(H, W, 0.35, 1)), ("noise45", noise(H, W, 0.45, 2)), ("noise60", noise(H, W, 0.6, 3)),
           ("blobs", blobs(H, W)), ("empty", np.zeros((H, W), bool))]
    return [(k, np.ascontiguousarray(m)) for k, m in out]


SHAPES = [(1, 1), (1, 70), (70, 1), (2, 2), (5, 63), (5, 64), (5, 65), (37, 127), (40, 129), (33, 300), (513, 513)]


def wake_cases():
    """solid inputs whose inner tiles go to sleep while the fronts are far away and must wake up when they arrive"""
    return [("stair240", stair(240)), ("stair288", stair(288)), ("full240", full(240, 240)), ("full250x245", full(250, 245)),
            ("full288", full(288, 288))]


def solid_cases():
    """the wake-up inputs and the solid shapes that converge without a tile ever waking"""
    return wake_cases() + [("stair240_slash", np.ascontiguousarray(stair(240).T[::-1])), ("full16x200", full(16, 200)),
                           ("full200x16", full(200, 16)), ("disc110", disc(221, 221, 110)), ("triangle240", triangle(240, 240, 240))]


# ------------------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------------------
def ref_labels(mask):
    """(H, W) i32: the smallest flat index of the pixel's 8-connected component, -1 on the background"""
    mask = np.asarray(mask, bool)
    lab, n = ndi.label(mask, EIGHT)
    idx = np.arange(mask.size, dtype=np.int64).reshape(mask.shape)
    roots = np.asarray(ndi.minimum(idx, lab, np.arange(1, n + 1)), np.int64).reshape(n)
    return np.where(lab > 0, np.concatenate([[-1], roots])[lab], -1).astype(np.int32)


def perimeter_codes(mask):
    """(3, H, W) bool: the pixels skimage's perimeter (4-neighbourhood) counts with weight 1, sqrt 2 and (1 + sqrt 2) / 2.  Computed
    on the whole mask at once: two 8-components are never adjacent, so no 3 x 3 window sees pixels of two of them."""
    m = np.asarray(mask, bool).astype(np.uint8)
    border = m - ndi.binary_erosion(m, morph._CROSS, border_value=0).astype(np.uint8)
    code = ndi.convolve(border, np.array([[10, 2, 10], [2, 1, 2], [10, 2, 10]]), mode="constant", cval=0)
    return np.stack([np.isin(code, c) for c in ((5, 7, 15, 17, 25, 27), (21, 33), (13, 23))])


def ref_stats(mask):
    """(4, H, W) i32: area, n1, n2, n3 of every component at its root pixel, 0 elsewhere"""
    mask = np.asarray(mask, bool)
    lab = ref_labels(mask)
    out = np.zeros((4, mask.size), np.int64)
    roots = lab[mask]
    planes = [np.ones(mask.shape, bool)] + list(perimeter_codes(mask))
    for j, pl in enumerate(planes):
        cnt = np.bincount(roots, weights=pl[mask].astype(np.float64), minlength=mask.size)
        out[j] = np.rint(cnt).astype(np.int64)
    return out.reshape((4,) + mask.shape).astype(np.int32)


def launch_trace(mask, with_skeleton=False):
    """The oracle's thinning iteration (the loop of oracle.morph.skeletonize_zhang, same table, same neighbour weights, both
    sub-iterations synchronous; the 3 x 3 code summed from shifted views instead of ndi.correlate, which is what makes 513 x 513
    affordable) in groups of ZH_IT full iterations, the work of one launch of zhang_tile_kernel.  Returns one (tiles_y, tiles_x)
    bool array per launch, True where a pixel of that ZH_TI-px tile was removed; the last entry is the launch that removes nothing.
    with_skeleton: also the converged skeleton (tests/test_morph_cases.py holds it against skeletonize_zhang itself)."""
    lut = morph.zhang_lut()
    H, W = mask.shape
    P = np.pad(np.asarray(mask, bool).astype(np.uint8), 1)
    c = P[1:-1, 1:-1]
    nb = ((P[:-2, :-2], 0), (P[:-2, 1:-1], 1), (P[:-2, 2:], 2), (P[1:-1, 2:], 3), (P[2:, 2:], 4), (P[2:, 1:-1], 5), (P[2:, :-2], 6),
          (P[1:-1, :-2], 7))                                  # NW N NE E SE S SW W = bits 0..7
    ty, tx = -(-H // ZH_TI), -(-W // ZH_TI)
    trace = []
    while True:
        before = c.copy()
        for sub in range(2 * ZH_IT):
            code = np.zeros((H, W), np.uint8)
            for v, k in nb:
                code |= v << k
            val = lut[code]
            c[(c > 0) & ((val == 3) | (val == (1 if sub % 2 == 0 else 2)))] = 0
        removed = before != c
        tiles = np.zeros((ty * ZH_TI, tx * ZH_TI), bool)
        tiles[:H, :W] = removed
        trace.append(tiles.reshape(ty, ZH_TI, tx, ZH_TI).any(axis=(1, 3)))
        if not removed.any():
            break
    return (trace, c.astype(bool)) if with_skeleton else trace


def launch_budget(H, W):
    """the removing launches filter_mask_dev allows before it reports `did not converge`"""
    return -(-(max(H, W) // 2 + 8) // ZH_IT)


def woken_tiles(trace):
    """(tiles_y, tiles_x) bool: tiles that went to sleep and had to wake.  A tile sleeps in launch j >= 1 when no tile of its 3 x 3
    tile neighbourhood removed anything in launch j - 1 (zhang_tile_kernel returns early); it has to wake when it removes
    something in a later launch."""
    slept = np.zeros_like(trace[0])
    woken = np.zeros_like(trace[0])
    for j in range(1, len(trace)):
        woken |= slept & trace[j]
        slept |= ~ndi.binary_dilation(trace[j - 1], EIGHT)
    return woken
