"""Inputs of the cell-area batch tests (tests/test_gpu_cellarea_batch.py): small seeded Z stacks whose slices differ enough that the
order of max projection and down-sampling matters, and well plates with independent cells per slice.

blob_stack: per slice, background 0.1 + N(0, 0.01) plus gaussian-blurred sparse blobs (p = 0.004, sigma 2.5, gain 40), scaled to
60 000 (uint16) or 250 (uint8).  For the shapes of the tests the max of the resized slices differs from the resized max in hundreds
of pixels, and slice 0 alone gives another picture again (asserted there).

well_plate: tests/test_gpu_cellarea.py:_well_plate extended to Z slices (the well and its background level on every slice, noise and
cells drawn per slice).  kind "round": a disc; "square": the rounded square u^8 + v^8 < 1; "noise": RandomState(9).uniform() * 60000,
in which the oracle finds no hull and returns the circle of get_circ_mask.
"""
import functools

import numpy as np


def blob_stack(seed, Z, H, W, dtype=np.uint16):
    from scipy import ndimage as ndi
    rs = np.random.RandomState(seed)
    top = 60000 if np.dtype(dtype) == np.uint16 else 250
    a = np.empty((Z, H, W), np.float64)
    for z in range(Z):
        a[z] = 0.1 + rs.normal(0, 0.01, (H, W)) + ndi.gaussian_filter((rs.uniform(size=(H, W)) < 0.004).astype(float), 2.5) * 40
    return np.clip(a / a.max() * top, 0, top).astype(dtype)


def well_plate(seed, kind="round", Z=3, shape=(300, 320), dtype=np.uint16):
    from scipy import ndimage as ndi
    if kind == "noise":
        return (np.random.RandomState(9).uniform(size=(Z,) + tuple(shape)) * 60000).astype(dtype)
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    if kind == "round":
        inside = (xx - shape[1] * 0.5) ** 2 + (yy - shape[0] * 0.52) ** 2 < (min(shape) * 0.43) ** 2
    else:
        u, v = (xx - shape[1] * 0.5) / (min(shape) * 0.43), (yy - shape[0] * 0.52) / (min(shape) * 0.43)
        inside = u ** 8 + v ** 8 < 1
    a = np.empty((Z,) + tuple(shape), np.float64)
    for z in range(Z):
        blobs = ndi.gaussian_filter((rs.uniform(size=shape) < 0.002).astype(float), 4) * 120
        a[z] = np.where(inside, 0.35, 0.05) + rs.normal(0, 0.01, shape) + np.where(inside, blobs, 0)
    top = 60000 if np.dtype(dtype) == np.uint16 else 250
    return np.clip(a / a.max() * top, 0, top).astype(dtype)


DSAMP_WELL, SD_WELL, SEED_WELL = 256, 0.25, 7


@functools.lru_cache(maxsize=None)
def well_batch(dtype="uint16"):
    """(3, 3, 300, 320): uint16 -- a round well, a rounded square, uniform noise; uint8 -- three round wells"""
    if dtype == "uint16":
        a = np.stack([well_plate(1, "round"), well_plate(2, "square"), well_plate(0, "noise")])
    else:
        a = np.stack([well_plate(3 + i, "round", dtype=np.uint8) for i in range(3)])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def well_oracle(dtype="uint16"):
    """oracle/cellarea.py:cell_area_well per stack of well_batch(dtype): [(area, thresholded, well)], computed once"""
    from oracle import cellarea as oc
    return [oc.cell_area_well(st, DSAMP_WELL, SD_WELL, seed=SEED_WELL) for st in well_batch(dtype)]
