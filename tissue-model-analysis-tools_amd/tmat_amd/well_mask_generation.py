"""Well detection (`--detect-well`): the reference's fl_tissue_model_tools/well_mask_generation.py (same function names and
arguments) over the C-ABI.

The pixel stages run on the GPU -- `auto_threshold_well` (gaussian, uint8 rescale, corner medians, Otsu threshold, disk(5)
erosion) is one call, tmat_well_threshold, and the two `skimage.feature.canny` calls are tmat_canny_mask.  Host code keeps
what the reference does on a <= 200-pixel image with library calls: the nearest-neighbour rescale (index arithmetic),
scipy.spatial.ConvexHull (the reference's own dependency), the hull mask (exact integer point-in-polygon test in place of
Delaunay.find_simplex), and the random superellipse search (:16-91), restated line by line with numpy.

The reference draws its 25 000 candidates from the GLOBAL numpy generator and never seeds it (:35), so two runs of the
reference give different masks.  Here the draw is `numpy.random.RandomState(seed).rand(num_iters, 6)` with an explicit `seed`
(scripts: --well-seed, default 0): the same stream the reference consumes after `numpy.random.seed(seed)`.

Batched form (`make_well_masks_batch`, used by branches.analyze_batch_well): the per-image steps above stay as they are; the random
search (tmat_superellipse_search: one thread per candidate, all images of the batch in one launch) and the two superellipse
rasterisations with the nearest resize (tmat_superellipse_masks, tmat_resize_nearest_u8) run on the GPU once per batch.  The device
decides a candidate / pixel only when it is certain (include/tmat.h); the rest is evaluated here with the reference's expression.

scikit-image version note (reference pins 0.22.0): `rescale` / `resize` with order 0 follow scipy.ndimage.zoom(order=0,
grid_mode=True), i.e. source index floor((i + 0.5) * n_in / n_out); canny follows the 0.18.3 source (magnitude by hypot).
"""
from __future__ import annotations

from numbers import Integral

import numpy as np

from . import _lib
from .sato import ensure_gaussian_table

SUPERELLIPSE_BOUNDS = np.array([
    (-np.pi / 20, np.pi / 20),   # theta
    (0.67, 1.33),                # d
    (0.9, 1.1),                  # s_a
    (0.9, 1.1),                  # s_b
    (-0.3, 0.3),                 # c_x
    (-0.3, 0.3),                 # c_y
])


def _gamma(x: float) -> float:
    from scipy.special import gamma          # the reference's own call (:10, :79-82)
    return gamma(x)


def get_superellipse_hull(x, y, n, num_iters=25000, seed=0):
    """Find a superellipse that encloses the given points (reference :16-91).  Returns (t, d, s_a, s_b, c_x, c_y); raises
    ValueError when no candidate encloses them (the reference's np.argmin of an empty sequence)."""
    linear_weights = np.random.RandomState(seed).rand(num_iters, 6)
    param_values = (SUPERELLIPSE_BOUNDS[:, 1] - SUPERELLIPSE_BOUNDS[:, 0]) * linear_weights + SUPERELLIPSE_BOUNDS[:, 0]
    t, d, s_a, s_b, c_x, c_y = param_values.T[..., np.newaxis]
    if n == 2:
        val = ((x - c_x) / (d * s_a)) ** 2 + ((y - c_y) / (d * s_b)) ** 2
    elif n % 2 == 0:
        val = ((((x - c_x) * np.cos(t) - ((y - c_y) * np.sin(t))) / (d * s_a)) ** n
               + (((x - c_x) * np.sin(t) + (y - c_y) * np.cos(t)) / (d * s_b)) ** n)
    else:
        val = (np.abs(((x - c_x) * np.cos(t) - ((y - c_y) * np.sin(t))) / (d * s_a)) ** n
               + np.abs(((x - c_x) * np.sin(t) + (y - c_y) * np.cos(t)) / (d * s_b)) ** n)
    candidate_indices = np.where(np.max(val, axis=1) < 1)[0]
    t, d, s_a, s_b, c_x, c_y = (q[candidate_indices] for q in (t, d, s_a, s_b, c_x, c_y))
    smallest_area_idx = np.argmin(4 * d ** 2 * s_a * s_b * _gamma(1 + 1 / n) ** 2 / _gamma(1 + 2 / n))
    return tuple(q[smallest_area_idx][0] for q in (t, d, s_a, s_b, c_x, c_y))


def gen_superellipse_mask(t, d, s_a, s_b, c_x, c_y, n, shape) -> np.ndarray:
    """reference :94-118"""
    x = np.linspace(-1, 1, shape[0])
    y = np.linspace(-1, 1, shape[1])
    X, Y = np.meshgrid(x, y)
    mask = ((np.abs(((X - c_x) * np.cos(t) - (Y - c_y) * np.sin(t)) / (d * s_a))) ** n
            + (np.abs(((X - c_x) * np.sin(t) + (Y - c_y) * np.cos(t)) / (d * s_b))) ** n
            < 1)
    return np.swapaxes(mask, 0, 1)


def create_convex_hull_mask(array_shape, hull_vertices) -> np.ndarray:
    """reference :121-139 (Delaunay(hull_vertices).find_simplex(all pixels) >= 0): the pixels inside or on the convex
    polygon, by exact integer cross products against every edge"""
    v = np.asarray(hull_vertices, np.int64)
    rr, cc = np.indices(array_shape)
    k = len(v)
    area2 = sum(int(v[i][0]) * int(v[(i + 1) % k][1]) - int(v[(i + 1) % k][0]) * int(v[i][1]) for i in range(k))
    sign = 1 if area2 > 0 else -1
    mask = np.ones(array_shape, bool)
    for i in range(k):
        a, b = v[i], v[(i + 1) % k]
        mask &= ((b[0] - a[0]) * (cc - a[1]) - (b[1] - a[1]) * (rr - a[0])) * sign >= 0
    return mask


def _resize_nearest(a: np.ndarray, shape) -> np.ndarray:
    """skimage.transform.resize(a, shape, order=0, preserve_range=True): source index floor((i + 0.5) * n_in / n_out)"""
    a = np.asarray(a)
    idx = [np.minimum(np.floor((np.arange(o) + 0.5) * (i / o)).astype(np.int64), i - 1) for o, i in zip(shape, a.shape)]
    return a[np.ix_(idx[0], idx[1])]


def _border(handle, mask: np.ndarray) -> np.ndarray:
    """canny(mask) plus the mask's pixels on the image border (reference :165-170, :201-205)"""
    m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
    ensure_gaussian_table(handle, 1.0, 0, 4.0)
    edges = np.empty_like(m)
    _lib.check(_lib.lib().tmat_canny_mask(handle.raw, _lib.ptr(m), m.shape[0], m.shape[1], 1.0, _lib.ptr(edges)), "tmat_canny_mask")
    b = edges.astype(bool)
    mb = m.astype(bool)
    b[0, :] |= mb[0, :]; b[-1, :] |= mb[-1, :]; b[:, 0] |= mb[:, 0]; b[:, -1] |= mb[:, -1]
    return b


def auto_threshold_well(image: np.ndarray, handle: _lib.Handle) -> np.ndarray:
    """Threshold an image to get a rough mask of the well (reference :236-277), on the GPU"""
    image = np.asarray(image)
    if image.ndim != 2:
        raise ValueError("auto_threshold_well: 2-D image expected")
    ensure_gaussian_table(handle, 1.0, 0, 4.0)
    out = np.empty(image.shape, np.uint8)
    if image.dtype == np.float32:
        img = np.ascontiguousarray(image)
        _lib.check(_lib.lib().tmat_well_threshold(handle.raw, _lib.ptr(img), img.shape[0], img.shape[1], _lib.ptr(out)), "tmat_well_threshold")
    else:
        # skimage's gaussian() converts with img_as_float: unsigned integers are multiplied by 1 / max in float64
        if image.dtype.kind == "u":
            img = np.multiply(image, 1.0 / np.iinfo(image.dtype).max, dtype=np.float64)
        elif image.dtype == np.float64:
            img = np.ascontiguousarray(image)
        else:
            raise ValueError("auto_threshold_well: float32 / float64 / unsigned integer images")
        _lib.check(_lib.lib().tmat_well_threshold_f64(handle.raw, _lib.ptr(img), img.shape[0], img.shape[1], _lib.ptr(out)), "tmat_well_threshold_f64")
    return out.astype(bool)


def generate_well_mask(image: np.ndarray, mask_val: Integral = 1, return_superellipse_params: bool = False, *,
                       handle: _lib.Handle, seed: int = 0):
    """Generate a binary mask over the well in an image (reference :142-233)."""
    from scipy.spatial import ConvexHull
    try:
        from scipy.spatial import QhullError
    except ImportError:                                     # older scipy
        from scipy.spatial.qhull import QhullError
    image = np.asarray(image)
    im_thresh = auto_threshold_well(image, handle)
    downsamp_ratio = min(1, 200 / np.max(im_thresh.shape))
    small_shape = tuple(int(v) for v in np.round(np.asarray(im_thresh.shape) * downsamp_ratio))
    im_thresh = _resize_nearest(im_thresh, small_shape)
    border_points = np.argwhere(_border(handle, im_thresh))

    def get_circ_mask():
        circ_mask = np.zeros(image.shape, dtype=np.uint8)
        center = image.shape[0] // 2, image.shape[1] // 2
        radius = int(image.shape[0] * 0.5 * (1 - 0.95))
        rr, cc = np.indices(image.shape)
        circ_mask[(rr - center[0]) ** 2 + (cc - center[1]) ** 2 < radius ** 2] = mask_val      # skimage.draw.disk
        return circ_mask

    try:
        hull = ConvexHull(border_points)
    except (ValueError, QhullError):                        # QhullError derives from ValueError in the pinned scipy
        return get_circ_mask()
    hull_vertices = border_points[hull.vertices]
    well_mask = create_convex_hull_mask(im_thresh.shape, hull_vertices)
    well_mask_border = _border(handle, well_mask)
    area = np.sum(well_mask)
    perimeter = np.sum(well_mask_border)
    n = 8 if perimeter / area > .027 else 2
    x = hull_vertices[:, 0] / im_thresh.shape[0] * 2 - 1
    y = hull_vertices[:, 1] / im_thresh.shape[1] * 2 - 1
    found_superellipse = False
    try:
        t, d, s_a, s_b, c_x, c_y = get_superellipse_hull(x, y, n, seed=seed)
        d *= 0.9
        well_mask = gen_superellipse_mask(t, d, s_a, s_b, c_x, c_y, n, im_thresh.shape)
        found_superellipse = True
    except ValueError:
        print("Falling back to convex hull well mask.", flush=True)
    well_mask = well_mask.astype(np.uint8) * mask_val
    well_mask = _resize_nearest(well_mask, image.shape).astype(np.float64)          # skimage's resize returns floats
    if found_superellipse and return_superellipse_params:
        return well_mask, t, d, s_a, s_b, c_x, c_y, n
    return well_mask


def make_well_mask(img: np.ndarray, *, handle: _lib.Handle, seed: int = 0, warn=print):
    """scripts/compute_branches.py:109-141: (well_mask, shrunken_well_mask) as boolean arrays; the second one (a 10 % smaller
    superellipse, or the mask eroded by disk(5) when the fit failed) becomes the pruning mask"""
    res = generate_well_mask(img, return_superellipse_params=True, handle=handle, seed=seed)
    if isinstance(res, tuple):
        well_mask, t, d, s_a, s_b, c_x, c_y, n = res
        well_mask = well_mask > 0
        d *= 0.9
        shrunken_well_mask = gen_superellipse_mask(t, d, s_a, s_b, c_x, c_y, n, img.shape[:2])
    else:
        well_mask = res > 0
        shrunken_well_mask = _erode_disk5(well_mask)
    coverage = np.sum(well_mask) / well_mask.size
    if coverage < 0.4:
        warn(f"Well mask coverage is too low ({coverage * 100:.2f}%) so it will not be used for analysis.")
        well_mask = np.full(img.shape, True, dtype=bool)
        shrunken_well_mask = np.full(img.shape, True, dtype=bool)
    return well_mask, shrunken_well_mask


def _erode_disk5(mask: np.ndarray) -> np.ndarray:
    """skimage binary_erosion(mask, disk(5)) (border counts as set) of the fallback mask: 81 shifted ANDs"""
    m = np.asarray(mask, bool)
    H, W = m.shape
    pad = np.ones((H + 10, W + 10), bool)
    pad[5:5 + H, 5:5 + W] = m
    out = np.ones((H, W), bool)
    for dy in range(-5, 6):
        for dx in range(-5, 6):
            if dy * dy + dx * dx <= 25:
                out &= pad[5 + dy:5 + dy + H, 5 + dx:5 + dx + W]
    return out


# ---- batched form: the superellipse fit on the device (csrc/wellfit_kernels.hip) ----------------------------------------------------

_CANDIDATES = {}


def superellipse_candidates(seed: int = 0, num_iters: int = 25000) -> dict:
    """The random candidates of get_superellipse_hull (:35-45) for (seed, num_iters), drawn once: t, d, s_a, s_b, c_x, c_y as the
    (num_iters, 1) views the reference evaluates, and cos t, sin t, d * s_a, d * s_b from the reference's own numpy calls on them"""
    key = (int(seed), int(num_iters))
    if key not in _CANDIDATES:
        linear_weights = np.random.RandomState(seed).rand(num_iters, 6)
        param_values = (SUPERELLIPSE_BOUNDS[:, 1] - SUPERELLIPSE_BOUNDS[:, 0]) * linear_weights + SUPERELLIPSE_BOUNDS[:, 0]
        t, d, s_a, s_b, c_x, c_y = param_values.T[..., np.newaxis]
        _CANDIDATES.clear()                              # one draw is kept: a run uses one seed
        _CANDIDATES[key] = dict(t=t, d=d, s_a=s_a, s_b=s_b, c_x=c_x, c_y=c_y, cos=np.cos(t), sin=np.sin(t), da=d * s_a, db=d * s_b)
    return _CANDIDATES[key]


def superellipse_area(cand: dict, n: int) -> np.ndarray:
    """(num_iters,) areas by the reference's expression (:79-82), gamma factor of exponent n included"""
    n = int(n)
    d, s_a, s_b = cand["d"], cand["s_a"], cand["s_b"]
    return np.ascontiguousarray((4 * d ** 2 * s_a * s_b * _gamma(1 + 1 / n) ** 2 / _gamma(1 + 2 / n))[:, 0])


def superellipse_table(n: int, seed: int = 0, num_iters: int = 25000) -> np.ndarray:
    """(num_iters, 7) f64 table of tmat_superellipse_table: c_x, c_y, cos t, sin t, d s_a, d s_b, area (for exponent n)"""
    c = superellipse_candidates(seed, num_iters)
    cols = [c["c_x"][:, 0], c["c_y"][:, 0], c["cos"][:, 0], c["sin"][:, 0], c["da"][:, 0], c["db"][:, 0], superellipse_area(c, n)]
    return np.ascontiguousarray(np.stack(cols, axis=1), np.float64)


def _reference_max(cand: dict, rows, x, y, n: int) -> np.ndarray:
    """max over the points of the reference's value (:47-72) for the candidates `rows` only"""
    rows = np.asarray(rows, np.int64)
    c_x, c_y, da, db = (cand[k][rows] for k in ("c_x", "c_y", "da", "db"))
    cos, sin = cand["cos"][rows], cand["sin"][rows]
    if n == 2:
        val = ((x - c_x) / da) ** 2 + ((y - c_y) / db) ** 2
    elif n % 2 == 0:
        val = ((((x - c_x) * cos - ((y - c_y) * sin)) / da) ** n + (((x - c_x) * sin + (y - c_y) * cos) / db) ** n)
    else:
        val = (np.abs(((x - c_x) * cos - ((y - c_y) * sin)) / da) ** n + np.abs(((x - c_x) * sin + (y - c_y) * cos) / db) ** n)
    return np.max(val, axis=1)


def merge_band(best: int, accepted, area: np.ndarray) -> int:
    """The candidate np.argmin would return: the lowest (area, index) among the device's `best` (-1: none) and the banded candidates
    the host accepted.  ValueError when there is none (the reference's np.argmin of an empty sequence)."""
    pool = sorted({int(j) for j in accepted} | ({int(best)} if best >= 0 else set()))
    if not pool:
        raise ValueError("attempt to get argmin of an empty sequence")
    return min(pool, key=lambda j: (area[j], j))


def superellipse_search_raw(handle: _lib.Handle, points, n_exps, cap_band: int = 4096):
    """tmat_superellipse_search on the table the handle holds: points = [(x, y)] per image -> (best (n_imgs,) i32, band (k, 2) i32)"""
    offs = np.zeros(len(points) + 1, np.int32)
    offs[1:] = np.cumsum([len(p[0]) for p in points])
    xy = np.ascontiguousarray(np.concatenate([np.stack([np.asarray(p[0], np.float64), np.asarray(p[1], np.float64)], axis=1) for p in points]))
    n_exp = np.ascontiguousarray(n_exps, np.int32)
    best = np.full(len(points), -2, np.int32)
    import ctypes as C
    L = _lib.lib()
    while True:
        band = np.zeros((max(cap_band, 1), 2), np.int32)
        n_band = C.c_int(0)
        rc = L.tmat_superellipse_search(handle.raw, _lib.ptr(xy), _lib.ptr(offs), len(points), _lib.ptr(n_exp), _lib.ptr(best), _lib.ptr(band),
                                        int(cap_band), C.byref(n_band))
        if rc == _lib.E_CAP and n_band.value > cap_band:            # the band list was too short: once more with what it needs
            cap_band = n_band.value
            continue
        _lib.check(rc, "tmat_superellipse_search")
        return best, band[: n_band.value].copy()


def superellipse_search_batch(handle: _lib.Handle, points, n_exps, seed: int = 0, num_iters: int = 25000):
    """get_superellipse_hull for a batch: points = [(x, y)] per image, n_exps = the exponent per image -> per image
    (t, d, s_a, s_b, c_x, c_y), or None where no candidate encloses the points.  One table upload and one search per distinct exponent
    (the area carries the exponent's gamma factor)."""
    cand = superellipse_candidates(seed, num_iters)
    out = [None] * len(points)
    L = _lib.lib()
    for n in sorted({int(v) for v in n_exps}):
        idx = [i for i, v in enumerate(n_exps) if int(v) == n]
        key = (int(seed), int(num_iters), n)
        table = None
        if getattr(handle, "_se_table_key", None) != key:
            table = superellipse_table(n, seed, num_iters)
            _lib.check(L.tmat_superellipse_table(handle.raw, _lib.ptr(table), int(num_iters)), "tmat_superellipse_table")
            handle._se_table_key = key
        area = superellipse_area(cand, n) if table is None else table[:, 6]
        best, band = superellipse_search_raw(handle, [points[i] for i in idx], [n] * len(idx))
        for k, i in enumerate(idx):
            rows = band[band[:, 0] == k, 1]
            accepted = rows[_reference_max(cand, rows, points[i][0], points[i][1], n) < 1] if len(rows) else []
            try:
                j = merge_band(int(best[k]), accepted, area)
            except ValueError:
                continue
            out[i] = tuple(cand[q][j][0] for q in ("t", "d", "s_a", "s_b", "c_x", "c_y"))
    return out


def get_superellipse_hull_dev(x, y, n, handle: _lib.Handle, num_iters: int = 25000, seed: int = 0):
    """get_superellipse_hull with the search on the device; raises ValueError when no candidate encloses the points"""
    res = superellipse_search_batch(handle, [(x, y)], [n], seed, num_iters)[0]
    if res is None:
        raise ValueError("attempt to get argmin of an empty sequence")
    return res


def gen_superellipse_masks_dev(handle: _lib.Handle, params, n_exps, shape, cap_band: int = 4096, return_band: bool = False):
    """gen_superellipse_mask for a batch of one shape on the device: params = [(t, d, s_a, s_b, c_x, c_y)], n_exps = the exponent per
    mask -> (len(params), shape[0], shape[1]) bool.  A mask with a pixel the device leaves undecided is evaluated again with the
    reference's expression on the reference's arrays.  return_band: also return the flat indices of those pixels."""
    import ctypes as C
    m = len(params)
    H, W = int(shape[0]), int(shape[1])
    out = np.zeros((m, H, W), np.uint8)
    if m == 0:
        return (out.astype(bool), np.zeros(0, np.int64)) if return_band else out.astype(bool)
    par = np.ascontiguousarray([[c_x, c_y, np.cos(t), np.sin(t), d * s_a, d * s_b] for t, d, s_a, s_b, c_x, c_y in params], np.float64)
    n_exp = np.ascontiguousarray(n_exps, np.int32)
    xs, ys = np.linspace(-1, 1, H), np.linspace(-1, 1, W)
    L = _lib.lib()
    while True:
        band = np.zeros(max(cap_band, 1), np.int64)
        n_band = C.c_int(0)
        rc = L.tmat_superellipse_masks(handle.raw, _lib.ptr(par), m, _lib.ptr(n_exp), _lib.ptr(xs), _lib.ptr(ys), H, W, _lib.ptr(out), _lib.ptr(band),
                                       int(cap_band), C.byref(n_band))
        if rc == _lib.E_CAP and n_band.value > cap_band:
            cap_band = n_band.value
            continue
        _lib.check(rc, "tmat_superellipse_masks")
        break
    out = out.astype(bool)
    for k in sorted({int(v) // (H * W) for v in band[: n_band.value]}):
        out[k] = gen_superellipse_mask(*params[k], int(n_exps[k]), (H, W))
    return (out, band[: n_band.value].copy()) if return_band else out


def resize_nearest_dev(handle: _lib.Handle, masks: np.ndarray, shape) -> np.ndarray:
    """_resize_nearest of a batch of masks (n, H, W) on the device -> (n, shape[0], shape[1]) u8"""
    a = np.ascontiguousarray(masks, np.uint8)
    out = np.empty((a.shape[0], int(shape[0]), int(shape[1])), np.uint8)
    _lib.check(_lib.lib().tmat_resize_nearest_u8(handle.raw, _lib.ptr(a), a.shape[0], a.shape[1], a.shape[2], out.shape[1], out.shape[2], _lib.ptr(out)),
               "tmat_resize_nearest_u8")
    return out


def small_shape_of(shape):
    """generate_well_mask :153-155: the shape the hull and the superellipse are searched on (tmat_well_small_shape)"""
    import ctypes as C
    sh, sw = C.c_int(), C.c_int()
    _lib.check(_lib.lib().tmat_well_small_shape(int(shape[0]), int(shape[1]), C.byref(sh), C.byref(sw)), "tmat_well_small_shape")
    return sh.value, sw.value


def _border_batch(handle, masks: np.ndarray) -> np.ndarray:
    """_border of k masks of one shape (k, h, w) through one tmat_canny_mask_batch call -> (k, h, w) bool"""
    m = np.ascontiguousarray(np.asarray(masks) != 0, np.uint8)
    if m.shape[0] == 0:
        return m.astype(bool)
    ensure_gaussian_table(handle, 1.0, 0, 4.0)
    edges = np.empty_like(m)
    _lib.check(_lib.lib().tmat_canny_mask_batch(handle.raw, _lib.ptr(m), m.shape[0], m.shape[1], m.shape[2], 1.0, _lib.ptr(edges)), "tmat_canny_mask_batch")
    b = edges.astype(bool)
    mb = m.astype(bool)
    b[:, 0, :] |= mb[:, 0, :]; b[:, -1, :] |= mb[:, -1, :]; b[:, :, 0] |= mb[:, :, 0]; b[:, :, -1] |= mb[:, :, -1]
    return b


def make_well_masks_batch(x, handle: _lib.Handle, seed: int = 0, warn=print):
    """make_well_mask for a batch of images of one shape: x (n, h, w), or a sequence of n (h, w) images (their dtypes may differ) ->
    (well (n, h, w) bool, shrunken (n, h, w) bool), equal to [make_well_mask(x[i]) for i].  Per image: threshold, nearest rescale, canny
    (generate_well_mask up to :170); the rest is make_well_masks_from_front."""
    x = [np.asarray(im) for im in x]
    if any(im.ndim != 2 or im.shape != x[0].shape for im in x):
        raise ValueError("make_well_masks_batch: 2-D images of one shape expected")
    if not x:
        return np.zeros((0, 0, 0), bool), np.zeros((0, 0, 0), bool)
    shape = x[0].shape
    downsamp_ratio = min(1, 200 / np.max(shape))
    small_shape = tuple(int(v) for v in np.round(np.asarray(shape) * downsamp_ratio))
    thresh_small = np.stack([_resize_nearest(auto_threshold_well(im, handle), small_shape) for im in x])
    border_small = np.stack([_border(handle, t) for t in thresh_small])
    return make_well_masks_from_front(thresh_small, border_small, shape, handle, seed, warn)


def _well_masks_from_front(thresh_small, border_small, shape, handle: _lib.Handle, seed: int, what: str):
    """generate_well_mask from the ConvexHull call on (:172-233) for a batch, the part make_well_masks_from_front and
    generate_well_masks_from_front share -> (well (n, h, w) bool, found, p_well, n_found): the well masks with generate_well_mask's own
    fallbacks (the circle of get_circ_mask without a hull, the hull mask without a fit), the images that have a superellipse, and its
    parameters (d already times 0.9) and exponent for each of those.  Per image: convex hull, hull mask; one batched canny for the hull
    masks' borders (the choice of the exponent), one superellipse search, one rasterisation + resize of the well masks for the batch."""
    from scipy.spatial import ConvexHull
    try:
        from scipy.spatial import QhullError
    except ImportError:                                     # older scipy
        from scipy.spatial.qhull import QhullError
    thresh_small, border_small = np.asarray(thresh_small), np.asarray(border_small)
    if thresh_small.ndim != 3 or border_small.shape != thresh_small.shape:
        raise ValueError(f"{what}: (n, sh, sw) masks and borders expected")
    n_img = len(thresh_small)
    small_shape = tuple(thresh_small.shape[1:])
    hull_of = {}                                            # image -> (small hull mask, hull vertices)
    for i in range(n_img):
        border_points = np.argwhere(border_small[i] != 0)
        try:
            hull = ConvexHull(border_points)
        except (ValueError, QhullError):
            continue
        hull_vertices = border_points[hull.vertices]
        hull_of[i] = (create_convex_hull_mask(small_shape, hull_vertices), hull_vertices)
    order = sorted(hull_of)
    hull_borders = _border_batch(handle, np.stack([hull_of[i][0] for i in order])) if order else []
    hulls = {}                                              # image -> (small hull mask, exponent, (x, y) of the hull vertices)
    for k, i in enumerate(order):
        hull_mask, hull_vertices = hull_of[i]
        n = 8 if np.sum(hull_borders[k]) / np.sum(hull_mask) > .027 else 2
        hulls[i] = (hull_mask, n, (hull_vertices[:, 0] / small_shape[0] * 2 - 1, hull_vertices[:, 1] / small_shape[1] * 2 - 1))
    fits = dict(zip(order, superellipse_search_batch(handle, [hulls[i][2] for i in order], [hulls[i][1] for i in order], seed))) if order else {}
    found = [i for i in order if fits[i] is not None]
    for i in order:
        if fits[i] is None:
            print("Falling back to convex hull well mask.", flush=True)
    # generate_well_mask: d *= 0.9, the mask at the small shape, resized
    p_well = [(t, d * 0.9, s_a, s_b, c_x, c_y) for t, d, s_a, s_b, c_x, c_y in (fits[i] for i in found)]
    n_found = [hulls[i][1] for i in found]
    small = {i: hulls[i][0] for i in order}
    if found:
        small.update(zip(found, gen_superellipse_masks_dev(handle, p_well, n_found, small_shape)))
    well = np.zeros((n_img,) + tuple(shape), bool)
    if order:
        well[order] = resize_nearest_dev(handle, np.stack([small[i] for i in order]), shape) > 0
    for i in range(n_img):
        if i not in hulls:                                  # get_circ_mask (:172-182)
            rr, cc = np.indices(shape)
            well[i] = (rr - shape[0] // 2) ** 2 + (cc - shape[1] // 2) ** 2 < int(shape[0] * 0.5 * (1 - 0.95)) ** 2
    return well, found, p_well, n_found


def generate_well_masks_from_front(thresh_small, border_small, shape, handle: _lib.Handle, seed: int = 0, mask_val: Integral = 255):
    """The tail of generate_well_mask (:172-233) for a batch: thresh_small, border_small (n, sh, sw) from tmat_cell_well_front_dev (or
    the per-image calls) and the images' shape -> (n, h, w) uint8 masks, 0 / mask_val, equal to [generate_well_mask(x[i], mask_val)].
    None of make_well_mask's rules applies here: a mask of low coverage stays as it is, and there is no shrunken mask."""
    shape = tuple(int(v) for v in shape)
    well = _well_masks_from_front(thresh_small, border_small, shape, handle, seed, "generate_well_masks_from_front")[0]
    return well.astype(np.uint8) * np.uint8(mask_val)


def make_well_masks_from_front(thresh_small, border_small, shape, handle: _lib.Handle, seed: int = 0, warn=print):
    """The tail of make_well_masks_batch, from the ConvexHull call on (generate_well_mask :172-233, make_well_mask): thresh_small,
    border_small (n, sh, sw) -- every image's thresholded mask at the small shape and its border (canny + the mask's pixels on the image
    border), from the per-image calls or from tmat_stack_well_front_dev -- and the images' shape -> (well (n, h, w) bool, shrunken
    (n, h, w) bool).  The well masks are _well_masks_from_front's; then make_well_mask's rules: one rasterisation of the shrunken masks
    for the whole batch (d *= 0.9 once more, at the image shape), the eroded mask where the fit failed, the coverage rule."""
    shape = tuple(int(v) for v in shape)
    well, found, p_well, n_found = _well_masks_from_front(thresh_small, border_small, shape, handle, seed, "make_well_masks_from_front")
    p_shrunk = [(t, d * 0.9, s_a, s_b, c_x, c_y) for t, d, s_a, s_b, c_x, c_y in p_well]
    shrunken = np.zeros_like(well)
    if found:
        shrunken[found] = gen_superellipse_masks_dev(handle, p_shrunk, n_found, shape)
    for i in range(len(well)):
        if i not in found:
            shrunken[i] = _erode_disk5(well[i])
        coverage = np.sum(well[i]) / well[i].size
        if coverage < 0.4:
            warn(f"Well mask coverage is too low ({coverage * 100:.2f}%) so it will not be used for analysis.")
            well[i] = True
            shrunken[i] = True
    return well, shrunken
