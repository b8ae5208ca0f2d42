"""GPU: the superellipse fit of well detection on the device (csrc/wellfit_kernels.hip) against oracle/wellmask.py: the batched random
search, the rasterisation, the nearest resize and make_well_masks_batch, through the C-ABI on a handle without a model.

The device decides a candidate (a pixel) for n != 2 only when its value is further than 1e-12 from 1 and hands the rest to numpy.  Every
comparison below therefore also asserts that the oracle's own values keep clear of that band (and that the device reported nothing),
so that a pass never comes from the host's adjudication alone -- except in the one case constructed to land in the band."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = np.load(Path(__file__).parent / "golden" / "wellmask.npz")
BAND = 1e-12


@pytest.fixture(scope="module")
def plain():
    from tmat_amd import _lib
    h = _lib.Handle(None, 0)
    yield h
    h.close()


def _points(npts):
    """npts points inside a radius of 0.5 around (0.04, -0.03): many of the candidates enclose them, many do not"""
    rs = np.random.RandomState(100 + npts)
    a, r = rs.uniform(0, 2 * np.pi, npts), rs.uniform(0.2, 0.5, npts)
    return r * np.cos(a) + 0.04, 0.9 * r * np.sin(a) - 0.03


def _oracle_max(x, y, n, seed, num_iters):
    """max over the points of the oracle's value per candidate: the lines of oracle/wellmask.py:get_superellipse_hull"""
    from oracle import wellmask as ow
    w = np.random.RandomState(seed).rand(num_iters, 6)
    pv = (ow.SUPERELLIPSE_BOUNDS[:, 1] - ow.SUPERELLIPSE_BOUNDS[:, 0]) * w + ow.SUPERELLIPSE_BOUNDS[:, 0]
    t, d, s_a, s_b, c_x, c_y = pv.T[..., np.newaxis]
    if n == 2:
        val = ((x - c_x) / (d * s_a)) ** 2 + ((y - c_y) / (d * s_b)) ** 2
    elif n % 2 == 0:
        val = ((((x - c_x) * np.cos(t) - ((y - c_y) * np.sin(t))) / (d * s_a)) ** n
               + (((x - c_x) * np.sin(t) + (y - c_y) * np.cos(t)) / (d * s_b)) ** n)
    else:
        val = (np.abs(((x - c_x) * np.cos(t) - ((y - c_y) * np.sin(t))) / (d * s_a)) ** n
               + np.abs(((x - c_x) * np.sin(t) + (y - c_y) * np.cos(t)) / (d * s_b)) ** n)
    return np.max(val, axis=1)


def _near_one(x, y, n, seed, num_iters):
    """How many candidates of the oracle have a value within BAND of 1, without a second pass of pow over (num_iters, points) values:
    the powers by squaring and multiplying, at most (n - 1) 2^-53 <= 1e-15 relative per term from pow's, counted within 2 * BAND --
    no candidate there means none of the oracle's within BAND.  n = 2 is the oracle's own expression."""
    if n == 2:
        return int(np.sum(np.abs(_oracle_max(x, y, n, seed, num_iters) - 1) <= BAND))
    from oracle import wellmask as ow
    w = np.random.RandomState(seed).rand(num_iters, 6)
    pv = (ow.SUPERELLIPSE_BOUNDS[:, 1] - ow.SUPERELLIPSE_BOUNDS[:, 0]) * w + ow.SUPERELLIPSE_BOUNDS[:, 0]
    t, d, s_a, s_b, c_x, c_y = pv.T[..., np.newaxis]

    def ipow(a):
        out, k = None, n
        while k:
            if k & 1:
                out = a if out is None else out * a
            a, k = a * a, k >> 1
        return out
    val = (ipow(np.abs(((x - c_x) * np.cos(t) - ((y - c_y) * np.sin(t))) / (d * s_a)))
           + ipow(np.abs(((x - c_x) * np.sin(t) + (y - c_y) * np.cos(t)) / (d * s_b))))
    return int(np.sum(np.abs(np.max(val, axis=1) - 1) <= 2 * BAND))


_ORACLE = {}


def _oracle(npts, n, seed, num_iters):
    """(oracle.wellmask.get_superellipse_hull of _points(npts), or None; candidates of the oracle inside the band), computed once"""
    from oracle import wellmask as ow
    key = (npts, n, seed, num_iters)
    if key not in _ORACLE:
        x, y = _points(npts)
        try:
            res = ow.get_superellipse_hull(x, y, n, seed, num_iters)
        except ValueError:
            res = None
        _ORACLE[key] = (res, _near_one(x, y, n, seed, num_iters))
    return _ORACLE[key]


# every point count with every exponent, candidate count and seed; the oracle's answers are computed once and shared (_oracle)
CASES = [(seed, num_iters, n, npts) for seed in (0, 7) for num_iters in (1000, 25000) for n in (2, 8, 3) for npts in (1, 3, 64, 257, 1024)]


@pytest.mark.parametrize("seed, num_iters, n, npts", CASES)
def test_search_equals_the_oracle(plain, seed, num_iters, n, npts):
    from tmat_amd import well_mask_generation as wm
    want, in_band = _oracle(npts, n, seed, num_iters)
    assert in_band == 0, "the oracle's own values must keep clear of the band"
    x, y = _points(npts)
    got = wm.superellipse_search_batch(plain, [(x, y)], [n], seed, num_iters)[0]
    assert got == want and want is not None
    # ... and the device alone decided it: nothing undecided, best is that very candidate
    best, band = wm.superellipse_search_raw(plain, [(x, y)], [n])
    cand = wm.superellipse_candidates(seed, num_iters)
    assert len(band) == 0 and tuple(cand[q][best[0]][0] for q in ("t", "d", "s_a", "s_b", "c_x", "c_y")) == want


@pytest.mark.parametrize("seed, num_iters", [(0, 1000), (7, 25000)])
def test_search_of_a_mixed_batch_in_one_call(plain, seed, num_iters):
    from tmat_amd import well_mask_generation as wm
    counts, exps = [1, 3, 64, 257, 1024, 64], [8, 2, 3, 8, 2, 2]
    want = []
    for npts, n in zip(counts, exps):
        res, in_band = _oracle(npts, n, seed, num_iters)
        assert in_band == 0
        want.append(res)
    got = wm.superellipse_search_batch(plain, [_points(k) for k in counts], exps, seed, num_iters)
    assert got == want and None not in want
    # one C call with images of several point counts and exponents: rotation / power per image (the area column is the one uploaded last,
    # exponent 8, whose images must come out right)
    best, band = wm.superellipse_search_raw(plain, [_points(k) for k in counts], exps)
    cand = wm.superellipse_candidates(seed, num_iters)
    assert len(band) == 0
    for k in (0, 3):
        assert tuple(cand[q][best[k]][0] for q in ("t", "d", "s_a", "s_b", "c_x", "c_y")) == want[k]


def test_points_no_candidate_encloses(plain):
    from oracle import wellmask as ow
    from tmat_amd import well_mask_generation as wm
    x, y = np.array([2.0, -2.0, 0.0]), np.array([0.0, 0.1, 1.9])
    for n in (2, 8):
        with pytest.raises(ValueError):
            ow.get_superellipse_hull(x, y, n, 0)
        with pytest.raises(ValueError):
            wm.get_superellipse_hull_dev(x, y, n, plain, seed=0)
        best, band = wm.superellipse_search_raw(plain, [(x, y), _points(3)], [n, n])
        assert best[0] == -1 and best[1] >= 0 and len(band) == 0
    assert wm.superellipse_search_batch(plain, [(x, y), _points(3)], [2, 2], 0)[0] is None


def _raw_search(plain, x, y, n):
    from tmat_amd import _lib
    xy = np.ascontiguousarray(np.stack([x, y], axis=1), np.float64)
    offs, n_exp, best, band, n_band = np.array([0, len(x)], np.int32), np.array([n], np.int32), np.zeros(1, np.int32), np.zeros((16, 2), np.int32), C.c_int(0)
    return _lib.lib().tmat_superellipse_search(plain.raw, _lib.ptr(xy), _lib.ptr(offs), 1, _lib.ptr(n_exp), _lib.ptr(best), _lib.ptr(band), 16, C.byref(n_band))


def test_search_refuses_too_many_points_and_bad_exponents(plain):
    from tmat_amd import _lib, well_mask_generation as wm
    wm.superellipse_search_batch(plain, [_points(3)], [2], 0, 1000)            # a table is on the handle
    x, y = _points(1024)
    assert _raw_search(plain, x, y, 2) == 0
    assert _raw_search(plain, np.append(x, 0.0), np.append(y, 0.0), 2) == _lib.E_CAP
    assert _raw_search(plain, x[:5], y[:5], 0) == _lib.E_ARG
    assert _raw_search(plain, x[:5], y[:5], 65) == _lib.E_ARG
    assert _raw_search(plain, x[:5], y[:5], 64) == 0


def test_n2_points_on_a_candidates_boundary_agree_with_numpy(plain):
    """n = 2 has no band: a point at (c_x + d s_a, c_y) of candidate j has the value ((x - c_x) / (d s_a)) ** 2 = 1 up to the rounding of
    x, and the device takes numpy's side of `< 1` bit for bit"""
    from oracle import wellmask as ow
    from tmat_amd import well_mask_generation as wm
    seed, num_iters = 7, 25000
    cand = wm.superellipse_candidates(seed, num_iters)
    order = np.argsort(wm.superellipse_area(cand, 2), kind="stable")[:48]     # small candidates: whether j itself accepts the point decides the answer
    pts = [(np.array([cand["c_x"][j, 0] + cand["da"][j, 0]]), np.array([cand["c_y"][j, 0]])) for j in order]
    got = wm.superellipse_search_batch(plain, pts, [2] * len(pts), seed, num_iters)
    best, band = wm.superellipse_search_raw(plain, pts, [2] * len(pts))
    assert len(band) == 0
    sides = set()
    for j, (x, y), g in zip(order, pts, got):
        assert g == ow.get_superellipse_hull(x, y, 2, seed, num_iters)
        sides.add(bool(((x - cand["c_x"][j]) / cand["da"][j]) ** 2 + ((y - cand["c_y"][j]) / cand["db"][j]) ** 2 < 1))
    assert sides == {False, True}, "both sides of the comparison must occur among the constructed points"


@pytest.mark.parametrize("side", [-1, 1])
def test_n8_candidate_inside_the_band_is_adjudicated_by_numpy(plain, side):
    """the one constructed case: a point whose value for candidate j (the smallest of all, so that j's verdict decides the answer) lies
    5e-14 below / above 1: the device reports j as undecided, the merged answer is the oracle's"""
    from oracle import wellmask as ow
    from tmat_amd import well_mask_generation as wm
    seed, num_iters, n = 7, 25000, 8
    cand = wm.superellipse_candidates(seed, num_iters)
    j = int(np.argmin(wm.superellipse_area(cand, n)))
    target = 1 + side * 5e-14
    val = lambda s: float(wm._reference_max(cand, [j], np.array([cand["c_x"][j, 0] + s]), np.array([cand["c_y"][j, 0] + 0.3 * s]), n)[0])   # noqa: E731
    lo, hi = 0.0, 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if val(mid) < target:
            lo = mid
        else:
            hi = mid
    s = min((lo, hi), key=lambda v: abs(val(v) - target))
    x, y = np.array([cand["c_x"][j, 0] + s]), np.array([cand["c_y"][j, 0] + 0.3 * s])
    mx = _oracle_max(x, y, n, seed, num_iters)
    assert abs(mx[j] - 1) < 1e-13 and (mx[j] < 1) == (side < 0)
    assert np.sum(np.abs(mx - 1) <= BAND) == 1, "only the constructed candidate lies in the band"
    want = ow.get_superellipse_hull(x, y, n, seed, num_iters)
    got = wm.superellipse_search_batch(plain, [(x, y)], [n], seed, num_iters)[0]
    best, band = wm.superellipse_search_raw(plain, [(x, y)], [n])
    assert band.tolist() == [[0, j]] and best[0] != j
    assert got == want
    assert (got == tuple(cand[q][j][0] for q in ("t", "d", "s_a", "s_b", "c_x", "c_y"))) == (side < 0)


# ---- masks ------------------------------------------------------------------------------------------------------------------------

PARAMS = [(0.11, 0.81, 1.04, 0.93, 0.17, -0.12), (-0.14, 0.7, 0.95, 1.08, -0.21, 0.09), (0.0, 1.3, 1.1, 1.1, 0.0, 0.0)]


@pytest.mark.parametrize("shape", [(7, 5), (200, 173), (33, 640)])
@pytest.mark.parametrize("n", [2, 8])
def test_superellipse_masks_equal_the_oracle(plain, n, shape):
    from oracle import wellmask as ow
    from tmat_amd import well_mask_generation as wm
    for p in PARAMS:        # the oracle's own pixel values keep clear of the band
        X, Y = np.meshgrid(np.linspace(-1, 1, shape[0]), np.linspace(-1, 1, shape[1]))
        t, d, s_a, s_b, c_x, c_y = p
        val = ((np.abs(((X - c_x) * np.cos(t) - (Y - c_y) * np.sin(t)) / (d * s_a))) ** n
               + (np.abs(((X - c_x) * np.sin(t) + (Y - c_y) * np.cos(t)) / (d * s_b))) ** n)
        assert not np.any(np.abs(val - 1) <= BAND)
    got, band = wm.gen_superellipse_masks_dev(plain, PARAMS, [n] * 3, shape, return_band=True)
    assert len(band) == 0 and got.shape == (3,) + shape and got.dtype == bool
    for k, p in enumerate(PARAMS):
        ref = ow.gen_superellipse_mask(*p, n, shape)
        assert np.array_equal(got[k], ref), k
        assert k == 2 or 0 < ref.sum() < ref.size
    mixed = wm.gen_superellipse_masks_dev(plain, PARAMS, [8, 2, 3], shape)          # the exponent is per mask
    for k, nk in enumerate([8, 2, 3]):
        assert np.array_equal(mixed[k], ow.gen_superellipse_mask(*PARAMS[k], nk, shape))


def test_a_pixel_inside_the_band_is_reported_and_patched(plain):
    """a superellipse through a grid point: |x / 0.5|^8 at x = 0.5 is exactly 1 on the 5-point linspace, so numpy says `not < 1` and the
    device leaves that pixel to numpy"""
    from oracle import wellmask as ow
    from tmat_amd import well_mask_generation as wm
    p = (0.0, 0.5, 1.0, 1.0, 0.0, 0.0)
    got, band = wm.gen_superellipse_masks_dev(plain, [p], [8], (5, 5), return_band=True)
    assert set(band.tolist()) == {5 * 1 + 2, 5 * 3 + 2, 5 * 2 + 1, 5 * 2 + 3}
    assert np.array_equal(got[0], ow.gen_superellipse_mask(*p, 8, (5, 5)))


@pytest.mark.parametrize("src, dst", [((200, 173), (640, 553)), ((5, 7), (20, 21)), ((640, 553), (200, 173))])
def test_nearest_resize_equals_the_host_function(plain, src, dst):
    from tmat_amd import well_mask_generation as wm
    a = (np.random.RandomState(3).uniform(size=(3,) + src) < 0.5).astype(np.uint8) * np.array([1, 7, 255], np.uint8)[:, None, None]
    got = wm.resize_nearest_dev(plain, a, dst)
    for k in range(3):
        assert np.array_equal(got[k], wm._resize_nearest(a[k], dst)), k


def _groups():
    """the inputs of tests/golden/wellmask.npz, grouped into batches of one shape (float32, uint16 and uint8 images side by side)"""
    import make_goldens
    inputs = make_goldens.wellmask_inputs()
    names = sorted({str(k).rsplit("_s", 1)[0] for k in GOLD["names"]})
    assert sorted(inputs) == names
    groups = {}
    for k in names:
        groups.setdefault(inputs[k].shape, []).append(k)
    return inputs, sorted(groups.values())


@pytest.mark.parametrize("seed", [0, 7])
@pytest.mark.parametrize("group", range(3))
def test_make_well_masks_batch_equals_the_oracle(plain, group, seed):
    from oracle import wellmask as ow
    from tmat_amd import well_mask_generation as wm
    inputs, groups = _groups()
    assert len(groups) == 3 and sum(len(g) for g in groups) == 7
    names = groups[group]
    well, shrunk = wm.make_well_masks_batch([inputs[k] for k in names], plain, seed=seed, warn=lambda m: None)
    for i, k in enumerate(names):
        ref = ow.make_well_mask(inputs[k], seed=seed)
        assert np.array_equal(well[i], ref[0]) and np.array_equal(shrunk[i], ref[1]), (k, seed)
