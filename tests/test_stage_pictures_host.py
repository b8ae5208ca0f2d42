"""tmat_host_stage_pictures (the host twin of csrc/vis_kernels.hip) against the picture rule in numpy, bit for bit: save_vis of the
reference (compute_branches.py:74-78) as tmat_amd.branches has always evaluated it.  No GPU."""
import warnings

import numpy as np
import pytest

from tmat_amd import _lib


def rule(a):
    """per image: lo / hi over the non-NaN values; ((a - lo) / (hi - lo)) * 255 if hi != lo else clip(a, 0, 255); NaN -> 0; rint -> u8"""
    a = np.asarray(a)
    out = np.empty(a.shape, np.uint8)
    for i in range(a.shape[0]):
        x = a[i].astype(np.float64)
        with warnings.catch_warnings(), np.errstate(invalid="ignore"):
            warnings.simplefilter("ignore", RuntimeWarning)         # all-NaN slice
            lo, hi = np.nanmin(x), np.nanmax(x)
            v = ((x - lo) / (hi - lo)) * 255.0 if hi != lo else np.minimum(np.maximum(x, 0.0), 255.0)
        out[i] = np.rint(np.where(np.isnan(v), 0.0, v)).astype(np.uint8)
    return out


def cases():
    """(name, (n, h, w) array): shared with tests/test_gpu_stage_pictures.py"""
    rs = np.random.RandomState(7)
    out = [("u16_random_n3", rs.randint(0, 65536, (3, 40, 52)).astype(np.uint16)),
           ("u16_narrow_range", rs.randint(1000, 1300, (2, 33, 31)).astype(np.uint16)),
           ("f64_unit", rs.uniform(0, 1, (3, 40, 52))),
           ("f32_field", (rs.uniform(0, 1, (3, 33, 31)) ** 3 * 7.5).astype(np.float32)),
           ("f64_1x7", rs.uniform(-3, 3, (3, 1, 7))),
           ("u16_1x7", rs.randint(0, 65536, (3, 1, 7)).astype(np.uint16)),
           ("f64_33x31", rs.uniform(0, 1, (3, 33, 31))),
           ("u8_33x31", (rs.uniform(0, 1, (3, 33, 31)) > 0.5).astype(np.uint8)),
           ("f64_two_blocks", rs.uniform(0, 1, (2, 70, 61)))]          # 4270 pixels: more than one workgroup of 256 x 16
    for c in (0, 1, 300, -5):
        out.append((f"f64_constant_{c}", np.full((2, 9, 11), float(c))))
        out.append((f"f32_constant_{c}", np.full((2, 9, 11), c, np.float32)))
    for c in (0, 1, 300):
        out.append((f"u16_constant_{c}", np.full((2, 9, 11), c, np.uint16)))
    mixed = (rs.uniform(0, 1, (20, 24)) > 0.7).astype(np.uint8)
    out.append(("u8_mask_zero_one_mixed", np.stack([np.zeros_like(mixed), np.ones_like(mixed), mixed])))
    # lo 0, hi 510: an odd integer k lands on k / 2 = x.5 exactly -> ties to even
    ties = np.concatenate([[0.0, 510.0], np.arange(1, 510, 2, dtype=np.float64)])
    out.append(("f64_ties_to_even", ties.reshape(1, 1, -1)))
    nan = rs.uniform(0, 1, (4, 17, 19))
    nan[0, 0, 0] = np.nan                       # the first element
    nan[1, 5, 3:9] = np.nan
    nan[1, 16, 18] = np.nan
    nan[2] = np.nan                             # an all-NaN image
    nan[3, :, :] = 2.5
    nan[3, 0, 0] = np.nan                       # constant but for a NaN: the clip branch with a NaN in it
    out.append(("f64_nan", nan))
    nan32 = nan.astype(np.float32)
    out.append(("f32_nan", nan32))
    return out


CASES = cases()


def test_rule_is_the_staged_save_vis():
    """the rule above is branches.save_visualizations' arithmetic (clip to [lo, hi] first, nan_to_num last), for finite input and NaNs"""
    for name, a in CASES:
        for x in np.asarray(a, np.float64):
            with warnings.catch_warnings(), np.errstate(invalid="ignore"):
                warnings.simplefilter("ignore", RuntimeWarning)
                lo, hi = np.nanmin(x), np.nanmax(x)
                y = np.clip(x, lo, hi)
                y = (y - lo) / (hi - lo) * 255.0 if hi != lo else np.clip(y, 0, 255)
                ref = np.rint(np.nan_to_num(y)).astype(np.uint8)
            assert np.array_equal(ref, rule(x[None])[0]), name


@pytest.mark.parametrize("name, a", CASES, ids=[c[0] for c in CASES])
def test_host_stage_pictures_matches_the_rule(name, a):
    got = _lib.host_stage_pictures(a)
    assert got.dtype == np.uint8 and got.shape == a.shape
    assert np.array_equal(got, rule(a)), name


def test_ties_round_to_even():
    a = dict(CASES)["f64_ties_to_even"]
    got = _lib.host_stage_pictures(a)[0, 0]
    k = np.arange(1, 510, 2)
    assert np.array_equal(got[2:], np.where(((k - 1) // 2) % 2 == 0, (k - 1) // 2, (k + 1) // 2))        # k / 2 -> the even neighbour
    assert got[0] == 0 and got[1] == 255


def test_all_nan_image_is_all_zero_and_nan_pixels_are_zero():
    a = dict(CASES)["f64_nan"]
    got = _lib.host_stage_pictures(a)
    assert not got[2].any()
    assert got[0, 0, 0] == 0 and not got[1, 5, 3:9].any()
    assert got[0].max() == 255 and got[0].ravel()[1:].min() == 0           # the extrema ignore the NaN in front
    assert got[3, 0, 0] == 0 and (got[3].ravel()[1:] == 2).all()           # clip branch: rint(2.5) = 2


def test_single_image_and_bool_input():
    m = np.zeros((5, 6), bool)
    m[2, 3] = True
    got = _lib.host_stage_pictures(m)
    assert got.shape == (5, 6) and got[2, 3] == 255 and got.sum() == 255


def test_bad_arguments_are_refused():
    with pytest.raises(ValueError):
        _lib.host_stage_pictures(np.zeros((3, 4), np.int32))
    L = _lib.lib()
    a, out = np.zeros(4, np.float64), np.zeros(4, np.uint8)
    assert L.tmat_host_stage_pictures(_lib.ptr(a), 7, 1, 4, _lib.ptr(out)) == _lib.E_ARG
    assert L.tmat_host_stage_pictures(None, 2, 1, 4, _lib.ptr(out)) == _lib.E_ARG
