"""Host side of the Z-stack (Sato) branch of analyze_img (reference scripts/compute_branches.py:224-306).

The reference does this branch inline in analyze_img with scikit-image / scipy calls; here the pixel work runs in
libtmat_hip.so (csrc/sato_kernels.hip, csrc/stack_pipeline.cpp) and this module is the thin host mirror: it hands scipy's
gaussian kernel tables to the library, calls the C-ABI and shapes the results.  No CPU fallback.

Gaussian tables: scipy builds them with numpy.exp, whose float64 loop is CPU-dispatched (its AVX512 path and libm's exp
differ in the last bit at some taps).  `install_gaussian_tables` computes the tables exactly as
scipy/ndimage/_filters.py:_gaussian_kernel1d does -- with THIS host's numpy -- and registers them on the handle, so the
filters reproduce what the reference would compute on the same machine bit for bit.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._lib import STACK_PASS_BUDGET, STACK_PASS_MAX, Handle, Row, StackOpts, VesselStages, check, lib, ptr

SATO_SIGMAS = (1, 2, 3, 4, 5, 7, 9, 11, 13, 15)            # compute_branches.py:262
GAUSSIAN_DERIVATIVES, GRADIENT = 0, 1                      # TMAT_SATO_*: scikit-image >= 0.20 (the pinned 0.22.0) / <= 0.19
HESSIAN_FORMS = {"gaussian_derivatives": GAUSSIAN_DERIVATIVES, "gradient": GRADIENT}
NEAREST, REFLECT, MIRROR = 0, 1, 2


def gaussian_kernel1d(sigma: float, order: int, radius: int) -> np.ndarray:
    """scipy.ndimage._filters._gaussian_kernel1d(sigma, order, radius)[::-1], the weights gaussian_filter1d hands to
    correlate1d (scipy 1.13: _filters.py:177-206, 265-268)"""
    if order < 0:
        raise ValueError("order must be non-negative")
    exponent_range = np.arange(order + 1)
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    phi_x = phi_x / phi_x.sum()
    if order == 0:
        return np.ascontiguousarray(phi_x[::-1], np.float64)
    q = np.zeros(order + 1)
    q[0] = 1
    D = np.diag(exponent_range[1:], 1)
    P = np.diag(np.ones(order) / -sigma2, -1)
    Q_deriv = D + P
    for _ in range(order):
        q = Q_deriv.dot(q)
    q = (x[:, None] ** exponent_range).dot(q)
    return np.ascontiguousarray((q * phi_x)[::-1], np.float64)


def ensure_gaussian_table(handle: Handle, sigma: float, order: int, truncate: float):
    """register scipy's table for (sigma, order, radius = int(truncate sigma + 0.5)) on the handle, once"""
    done = getattr(handle, "_gauss_done", None)
    if done is None:
        done = handle._gauss_done = set()
    radius = int(truncate * float(sigma) + 0.5)
    key = (float(sigma), int(order), radius)
    if key in done:
        return
    w = gaussian_kernel1d(float(sigma), order, radius)
    check(lib().tmat_set_gaussian_table(handle.raw, float(sigma), order, radius, ptr(w)), "tmat_set_gaussian_table")
    done.add(key)


def install_gaussian_tables(handle: Handle, stack_hw=None, out_hw=None, sigmas=SATO_SIGMAS):
    """register every table the branch uses: sigma 1 and 2 (truncate 4), the Sato scales in both Hessian forms, and the
    anti-aliasing sigmas of the resize from stack_hw to out_hw"""
    ensure_gaussian_table(handle, 1.0, 0, 4.0)
    ensure_gaussian_table(handle, 2.0, 0, 4.0)
    sq1_2 = 1 / math.sqrt(2)
    for s in sigmas:
        ensure_gaussian_table(handle, float(s), 0, 4.0)          # gradient form
        tr = 8.0 if s > 1 else 100.0                             # corner.py:_hessian_matrix_with_gaussian
        ensure_gaussian_table(handle, sq1_2 * s, 0, tr)
        ensure_gaussian_table(handle, sq1_2 * s, 1, tr)
    if stack_hw is not None and out_hw is not None:
        for n_in, n_out in zip(stack_hw, out_hw):
            sg = max(0.0, (n_in / n_out - 1) / 2)
            if sg > 1e-15:
                ensure_gaussian_table(handle, sg, 0, 4.0)


def gaussian(handle: Handle, x: np.ndarray, sigma=1.0, mode=NEAREST) -> np.ndarray:
    """skimage.filters.gaussian on a float32 array of 2 or 3 dimensions"""
    x = np.ascontiguousarray(x, np.float32)
    if x.ndim not in (2, 3):
        raise ValueError("gaussian: 2-D or 3-D float32 input")
    ensure_gaussian_table(handle, sigma, 0, 4.0)
    d = (1,) + x.shape if x.ndim == 2 else x.shape
    out = np.empty_like(x)
    check(lib().tmat_gaussian_f32(handle.raw, ptr(x), d[0], d[1], d[2], float(sigma), int(mode), ptr(out)), "tmat_gaussian_f32")
    return out


def sato(handle: Handle, imgs: np.ndarray, sigmas=SATO_SIGMAS, hessian="gaussian_derivatives") -> np.ndarray:
    """skimage.filters.sato(img, sigmas, black_ridges=False) on one (h, w) or n (n, h, w) float32 images"""
    x = np.ascontiguousarray(imgs, np.float32)
    single = x.ndim == 2
    xb = x[None] if single else x
    install_gaussian_tables(handle, sigmas=tuple(sigmas))
    sg = np.ascontiguousarray(sigmas, np.float64)
    out = np.empty_like(xb)
    check(lib().tmat_sato_batch(handle.raw, ptr(xb), xb.shape[0], xb.shape[1], xb.shape[2], ptr(sg), len(sg), HESSIAN_FORMS[hessian], ptr(out)),
          "tmat_sato_batch")
    return out[0] if single else out


def dsamp_shape(shape, width=384):
    """img_dsamp_res (compute_branches.py:218-222)"""
    return tuple(int(v) for v in np.multiply(shape[-2:], width / shape[-1]).round().astype(int))


def _as_u16_stack(stack: np.ndarray) -> np.ndarray:
    stack = np.asarray(stack)
    if stack.ndim != 3 or stack.dtype not in (np.uint8, np.uint16):
        raise ValueError("Z stack: expected (Z, H, W) uint8 or uint16")
    return np.ascontiguousarray(stack, np.uint16)


def stack_prepare(handle: Handle, stack: np.ndarray, out_hw) -> np.ndarray:
    """compute_branches.py:247-256 -> (Z, out_h, out_w) float32 in 0..1"""
    a = _as_u16_stack(stack)
    install_gaussian_tables(handle, a.shape[1:], out_hw, sigmas=())
    vol = np.empty((a.shape[0],) + tuple(out_hw), np.float32)
    check(lib().tmat_stack_prepare(handle.raw, ptr(a), a.shape[0], a.shape[1], a.shape[2], out_hw[0], out_hw[1], ptr(vol)), "tmat_stack_prepare")
    return vol


def vessel_field(handle: Handle, vol: np.ndarray, hessian="gaussian_derivatives", return_stages=False):
    """compute_branches.py:258-302: prepared stack (Z, h, w) float32 -> vesselness image (h, w) float32"""
    v = np.ascontiguousarray(vol, np.float32)
    Z, h, w = v.shape
    install_gaussian_tables(handle)
    field = np.empty((h, w), np.float32)
    st = None
    arrays = {}
    if return_stages:
        st = VesselStages()
        for k in ("vess", "sharp"):
            arrays[k] = np.empty((Z - 1, h, w), np.float32)
        arrays["vessels"] = np.empty((h, w), np.float32)
        for k in ("edges", "skel", "mask_sel", "grown", "closed", "filt"):
            arrays[k] = np.empty((h, w), np.uint8)
        for k, a in arrays.items():
            setattr(st, k, a.ctypes.data)
    check(lib().tmat_vessel_field(handle.raw, ptr(v), Z, h, w, HESSIAN_FORMS[hessian], ptr(field), C.byref(st) if st is not None else None),
          "tmat_vessel_field")
    if return_stages:
        return field, {k: (a.astype(bool) if a.dtype == np.uint8 else a) for k, a in arrays.items()}
    return field


def vessel_field_batch(handle: Handle, vols: np.ndarray, hessian="gaussian_derivatives", return_stages=False):
    """tmat_vessel_field_batch: n prepared stacks (n, Z, h, w) float32 through one launch set -> fields (n, h, w) float32
    [, stages: the arrays of vessel_field with a leading n]"""
    v = np.ascontiguousarray(vols, np.float32)
    if v.ndim != 4:
        raise ValueError("vessel_field_batch: expected (n, Z, h, w)")
    n, Z, h, w = v.shape
    install_gaussian_tables(handle)
    fields = np.empty((n, h, w), np.float32)
    st = None
    arrays = {}
    if return_stages:
        st = VesselStages()
        for k in ("vess", "sharp"):
            arrays[k] = np.empty((n, Z - 1, h, w), np.float32)
        arrays["vessels"] = np.empty((n, h, w), np.float32)
        for k in ("edges", "skel", "mask_sel", "grown", "closed", "filt"):
            arrays[k] = np.empty((n, h, w), np.uint8)
        for k, a in arrays.items():
            setattr(st, k, a.ctypes.data)
    check(lib().tmat_vessel_field_batch(handle.raw, ptr(v), n, Z, h, w, HESSIAN_FORMS[hessian], ptr(fields), C.byref(st) if st is not None else None),
          "tmat_vessel_field_batch")
    if return_stages:
        return fields, {k: (a.astype(bool) if a.dtype == np.uint8 else a) for k, a in arrays.items()}
    return fields


def stack_pass_plan(n, Z, H, W, ds_width=384, pass_stacks=0):
    """tmat_stack_pass_plan (host only): (stacks per pass, device bytes per stack) of analyze_stack_batch for n stacks of (Z, H, W)"""
    k, b = C.c_int(), C.c_uint64()
    check(lib().tmat_stack_pass_plan(int(n), int(Z), int(H), int(W), int(ds_width), int(pass_stacks), C.byref(k), C.byref(b)), "tmat_stack_pass_plan")
    return k.value, b.value


def stacks_per_pass(n, bytes_per_stack, pass_stacks=0, budget=STACK_PASS_BUDGET, max_stacks=STACK_PASS_MAX):
    """the K rule of tmat_analyze_stack_batch (include/tmat.h): min(n, 8, budget // bytes per stack), at least 1; pass_stacks > 0 overrides"""
    if pass_stacks > 0:
        return max(1, min(n, pass_stacks))
    return max(1, min(n, max_stacks, budget // bytes_per_stack if bytes_per_stack else max_stacks))


def chunk_ends(cur_key, cur_len, cur_bytes, key, nbytes, budget=STACK_PASS_BUDGET, max_stacks=STACK_PASS_MAX):
    """does a chunk of cur_len stacks of cur_key holding cur_bytes end before a stack of (key, nbytes)?  (chunk_stacks, and the
    streaming loop of compute_branches.py)"""
    return key != cur_key or cur_len >= max_stacks or cur_bytes + nbytes > budget


def stack_chunk_bytes(shape, ds_width=384):
    """device bytes one stack of (Z, H, W) adds to a chunk of compute_branches.py's batch path: what a pass takes for it
    (tmat_stack_pass_plan) plus its uint16 copy in the chunk that stays resident for the whole call"""
    Z, H, W = (int(v) for v in shape)
    return stack_pass_plan(1, Z, H, W, ds_width)[1] + Z * H * W * 2


def stack_chunk_ends(held_keys, key, shape, ds_width=384, budget=STACK_PASS_BUDGET, max_stacks=STACK_PASS_MAX):
    """chunk_ends for the stream of loaded stacks: does the held chunk (held_keys, one key per stack, all equal) end before a stack of
    `key` and `shape`?  Every stack counts stack_chunk_bytes"""
    nb = stack_chunk_bytes(shape, ds_width)
    return chunk_ends(held_keys[0], len(held_keys), nb * len(held_keys), key, nb, budget, max_stacks)


def chunk_stacks(keys, nbytes, budget=STACK_PASS_BUDGET, max_stacks=STACK_PASS_MAX):
    """Grouping rule of compute_branches.py's Z-stack path, as a pure function.  keys[i]: what must be equal for stacks to share a batch
    call ((Z, H, W) and the width in microns); nbytes[i]: device bytes of stack i in a pass.  Consecutive stacks with equal keys form a
    chunk; a chunk ends when the next stack would take it past `budget` bytes or `max_stacks` stacks.  Order is preserved; a stack
    whose key differs from both neighbours is a chunk of one.  -> list of lists of indices"""
    chunks, cur, cur_bytes = [], [], 0
    for i, (key, nb) in enumerate(zip(keys, nbytes)):
        if cur and chunk_ends(keys[cur[0]], len(cur), cur_bytes, key, nb, budget, max_stacks):
            chunks.append(cur)
            cur, cur_bytes = [], 0
        cur.append(i)
        cur_bytes += nb
    if cur:
        chunks.append(cur)
    return chunks


class DevStacks:
    """n Z stacks of one shape resident in device memory: `ptr` (a tmat_dev_alloc block of n Z H W uint16) and `shape` (n, Z, H, W).
    upload_stacks makes one; analyze_stack_batch and stack_well_masks_batch take it in place of an array and only read it."""

    def __init__(self, handle: Handle, ptr_, shape):
        self.handle, self.ptr, self.shape = handle, ptr_, tuple(int(v) for v in shape)

    @property
    def nbytes(self):
        return int(np.prod(self.shape)) * 2

    def download(self) -> np.ndarray:
        out = np.empty(self.shape, np.uint16)
        check(lib().tmat_dev_download(self.handle.raw, ptr(out), self.ptr, out.nbytes), "tmat_dev_download")
        return out

    def free(self):
        if self.ptr is not None:
            check(lib().tmat_dev_free(self.handle.raw, self.ptr), "tmat_dev_free")
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def upload_stacks(handle: Handle, stacks) -> DevStacks:
    """(n, Z, H, W) uint8 / uint16 stacks -> DevStacks (one upload); free() it, or use it as a context manager"""
    a = np.asarray(stacks)
    if a.ndim != 4 or a.dtype not in (np.uint8, np.uint16):
        raise ValueError("Z stacks: expected (n, Z, H, W) uint8 or uint16")
    a = np.ascontiguousarray(a, np.uint16)
    d = C.c_void_p()
    check(lib().tmat_dev_alloc(handle.raw, a.nbytes, C.byref(d)), "tmat_dev_alloc")
    dev = DevStacks(handle, d, a.shape)
    try:
        check(lib().tmat_dev_upload(handle.raw, d, ptr(a), a.nbytes), "tmat_dev_upload")
    except Exception:
        dev.free()
        raise
    return dev


def _stacks_arg(stacks):
    """array, DevStacks or (device pointer, (n, Z, H, W)) -> (what the C entry takes, shape, resident?, the array to keep alive)"""
    if isinstance(stacks, DevStacks):
        return stacks.ptr, stacks.shape, True, None
    if isinstance(stacks, tuple) and len(stacks) == 2 and not isinstance(stacks[0], np.ndarray):
        shape = tuple(int(v) for v in stacks[1])
        if len(shape) != 4:
            raise ValueError("Z stacks on the device: expected (pointer, (n, Z, H, W))")
        return stacks[0], shape, True, None
    a = np.asarray(stacks)
    if a.ndim != 4 or a.dtype not in (np.uint8, np.uint16):
        raise ValueError("Z stacks: expected (n, Z, H, W) uint8 or uint16")
    a = np.ascontiguousarray(a, np.uint16)
    return ptr(a), a.shape, False, a


def analyze_stack_batch(handle: Handle, stacks, thresh_pairs, smoothing_window_px, min_branch_length_px, max_branch_length_px=None,
                        remove_isolated=False, ds_width=384, hessian="gaussian_derivatives", first_index=0, pruning_masks=None,
                        return_fields=False, return_pictures=False, pass_stacks=0, tree=False, vis_width=2000, overlays=True, cap_bars=4096):
    """tmat_analyze_stack_batch: n stacks of one shape (n, Z, H, W) and a list of (graph_thresh_1, graph_thresh_2) pairs ->
    rows[t][i] = (count, total_px, avg_px) of stack i at pair t [, fields (n, fh, fw) float32][, (projection pictures (n, H, W) uint8,
    field pictures (n, fh, fw) uint8)].  pruning_masks: None or (n, fh, fw) bool, MorseGraph's pruning mask per stack.
    stacks: an array, or stacks resident in device memory (a DevStacks, or (device pointer, shape)): tmat_analyze_stack_batch_dev, which
    leaves that buffer as it was.
    tree: the tree request of tmat_stack_opts; the last element of the result is then {"bars": bars[t][i] (k, 2) float64, scaled by
    W / fw as field_tree scales them, "overlays": (n_thresh, n, vh, vw, 3) uint8 or None (overlays=False: geometry only)}.  cap_bars: the
    bars an item may have in the first attempt; the call is repeated once with fh * fw, which always suffices"""
    src, shape, resident, _keep = _stacks_arg(stacks)
    n, Z, H, W = shape
    out_hw = dsamp_shape(shape, ds_width)
    install_gaussian_tables(handle, shape[2:], out_hw)
    th = np.ascontiguousarray(thresh_pairs, np.float32).reshape(-1, 2)
    o = StackOpts()
    o.size = C.sizeof(StackOpts)
    o.ds_width, o.hessian = int(ds_width), HESSIAN_FORMS[hessian]
    o.n_thresh, o.thresh = len(th), th.ctypes.data if len(th) else None
    o.smoothing_window_px, o.min_branch_length_px = int(smoothing_window_px), int(min_branch_length_px)
    o.max_branch_length_px, o.remove_isolated = int(max_branch_length_px or 0), int(bool(remove_isolated))
    o.first_index, o.pass_stacks = int(first_index), int(pass_stacks)
    pm = None
    if pruning_masks is not None:
        pm = np.ascontiguousarray(np.asarray(pruning_masks) > 0, np.uint8)
        if pm.shape != (n,) + tuple(out_hw):
            raise ValueError("analyze_stack_batch: pruning_masks must be (n,) + the field's shape")
        o.pruning_masks = pm.ctypes.data
    fields = np.empty((n,) + tuple(out_hw), np.float32) if return_fields else None
    if return_fields:
        o.fields_out = fields.ctypes.data
    pics = None
    if return_pictures:
        pics = (np.empty((n, H, W), np.uint8), np.empty((n,) + tuple(out_hw), np.uint8))
        o.proj_pic_out, o.field_pic_out = pics[0].ctypes.data, pics[1].ctypes.data
    rows = (Row * (max(len(th), 1) * n))()
    entry = lib().tmat_analyze_stack_batch_dev if resident else lib().tmat_analyze_stack_batch
    what = "tmat_analyze_stack_batch_dev" if resident else "tmat_analyze_stack_batch"
    T = max(len(th), 1)
    rgb = nb = bars = None
    if tree:
        from ._lib import E_CAP, tree_canvas_shape
        nb = np.zeros((T, n), np.int32)
        o.n_bars = nb.ctypes.data
        if overlays:
            vh, vw = tree_canvas_shape(H, W, vis_width)
            rgb = np.empty((T, n, vh, vw, 3), np.uint8)
            o.vis_width, o.rgb_out = int(vis_width), rgb.ctypes.data
        full = out_hw[0] * out_hw[1]          # a branch holds at least one vertex of its own
        for cap in (int(cap_bars), max(int(cap_bars), full)):
            bars = np.empty((T, n, cap, 2), np.float64)
            o.bars_out, o.cap_b = bars.ctypes.data, cap
            rc = entry(handle.raw, src, n, Z, H, W, C.byref(o), rows)
            if rc != E_CAP or cap >= full:
                break
        check(rc, what)
    else:
        check(entry(handle.raw, src, n, Z, H, W, C.byref(o), rows), what)
    res = ([[(rows[t * n + i].count, rows[t * n + i].total_px, rows[t * n + i].avg_px) for i in range(n)] for t in range(len(th))],)
    if return_fields:
        res += (fields,)
    if return_pictures:
        res += (pics,)
    if tree:
        res += ({"bars": [[bars[t, i, : nb[t, i]].copy() for i in range(n)] for t in range(len(th))], "overlays": rgb},)
    return res[0] if len(res) == 1 else res


def stack_trace(handle: Handle):
    """tmat_debug_stack_trace: [(device stages ms, host graph stage ms)] per pass of the handle's last analyze_stack_batch"""
    n = C.c_int()
    check(lib().tmat_debug_stack_trace(handle.raw, 0, C.byref(n), None, None), "tmat_debug_stack_trace")
    g, h = np.zeros(max(n.value, 1)), np.zeros(max(n.value, 1))
    check(lib().tmat_debug_stack_trace(handle.raw, n.value, C.byref(n), ptr(g), ptr(h)), "tmat_debug_stack_trace")
    return [(float(g[i]), float(h[i])) for i in range(n.value)]


def analyze_stack(handle: Handle, stack: np.ndarray, graph_thresh_1, graph_thresh_2, smoothing_window_px, min_branch_length_px,
                  max_branch_length_px=None, remove_isolated=False, ds_width=384, hessian="gaussian_derivatives", index=0, return_field=False):
    """tmat_analyze_stack: one Z stack -> (count, total_px, avg_px[, field])"""
    a = _as_u16_stack(stack)
    out_hw = dsamp_shape(a.shape, ds_width)
    install_gaussian_tables(handle, a.shape[1:], out_hw)
    row = Row()
    field = np.empty(out_hw, np.float32) if return_field else None
    check(lib().tmat_analyze_stack(handle.raw, ptr(a), a.shape[0], a.shape[1], a.shape[2], int(ds_width), HESSIAN_FORMS[hessian], float(graph_thresh_1),
                                   float(graph_thresh_2), int(smoothing_window_px), int(min_branch_length_px), int(max_branch_length_px or 0),
                                   int(bool(remove_isolated)), int(index), C.byref(row), ptr(field) if return_field else None), "tmat_analyze_stack")
    res = (row.count, row.total_px, row.avg_px)
    return res + (field,) if return_field else res


def field_stats(handle: Handle, field: np.ndarray, graph_thresh_1, graph_thresh_2, smoothing_window_px, min_branch_length_px,
                max_branch_length_px=None, remove_isolated=False, index=0, pruning_mask=None):
    """tmat_field_stats(_pruned): vesselness image -> (count, total_px, avg_px); pruning_mask (bool, the field's shape) is MorseGraph's
    `pruning_mask` (compute_branches.py:243, 412-420: the inverse of the shrunken well mask under --detect-well)"""
    f = np.ascontiguousarray(field, np.float32)
    row = Row()
    pm = None
    if pruning_mask is not None:
        pm = np.ascontiguousarray(np.asarray(pruning_mask) > 0, np.uint8)
        if pm.shape != f.shape:
            raise ValueError("field_stats: pruning_mask must have the field's shape")
    check(lib().tmat_field_stats_pruned(handle.raw, ptr(f), f.shape[0], f.shape[1], float(graph_thresh_1), float(graph_thresh_2), int(smoothing_window_px),
                                        int(min_branch_length_px), int(max_branch_length_px or 0), int(bool(remove_isolated)),
                                        ptr(pm) if pm is not None else None, int(index), C.byref(row)), "tmat_field_stats_pruned")
    return row.count, row.total_px, row.avg_px


def resize_aa(handle: Handle, imgs: np.ndarray, out_hw) -> np.ndarray:
    """skimage.transform.resize(x, out_hw, order=1, preserve_range=True, anti_aliasing=True) of one (H, W) or n (n, H, W) uint8 / uint16
    images -> float64 (compute_branches.py:232-238: the max projection of a Z stack before make_well_mask)"""
    a = np.asarray(imgs)
    single = a.ndim == 2
    a = _as_u16_stack(a[None] if single else a)
    install_gaussian_tables(handle, a.shape[1:], out_hw, sigmas=())
    out = np.empty((a.shape[0],) + tuple(int(v) for v in out_hw), np.float64)
    check(lib().tmat_resize_aa_u16(handle.raw, ptr(a), a.shape[0], a.shape[1], a.shape[2], int(out_hw[0]), int(out_hw[1]), ptr(out)), "tmat_resize_aa_u16")
    return out[0] if single else out


def stack_well_masks(handle: Handle, stack: np.ndarray, out_hw, seed=0):
    """--detect-well for a Z stack (compute_branches.py:227-243): well mask of the anti-alias-resized max projection
    -> (well_mask, pruning_mask) bool arrays of shape out_hw (pruning = not shrunken well)"""
    from . import well_mask_generation as wmg
    proj = np.asarray(stack).max(0)
    well, shrunken = wmg.make_well_mask(resize_aa(handle, proj, out_hw), handle=handle, seed=seed)
    return well, np.logical_not(shrunken)


def stack_well_front(handle: Handle, stacks, out_hw, return_proj=False):
    """tmat_stack_well_front_dev: the front end of --detect-well for n stacks of one shape in one launch set.  stacks: as
    analyze_stack_batch takes them (an array is uploaded for the call) -> (thresh_small, border_small) (n, sh, sw) uint8
    [, the anti-alias-resized max projections (n, out_h, out_w) float64]"""
    from . import well_mask_generation as wmg
    src, shape, resident, a = _stacks_arg(stacks)
    if not resident:
        with upload_stacks(handle, a) as dev:
            return stack_well_front(handle, dev, out_hw, return_proj)
    n, Z, H, W = shape
    out_hw = tuple(int(v) for v in out_hw)
    install_gaussian_tables(handle, (H, W), out_hw, sigmas=())
    sh, sw = wmg.small_shape_of(out_hw)
    thresh, border = np.empty((n, sh, sw), np.uint8), np.empty((n, sh, sw), np.uint8)
    proj = np.empty((n,) + out_hw, np.float64) if return_proj else None
    check(lib().tmat_stack_well_front_dev(handle.raw, src, n, Z, H, W, out_hw[0], out_hw[1], ptr(proj) if return_proj else None, ptr(thresh), ptr(border)),
          "tmat_stack_well_front_dev")
    return (thresh, border, proj) if return_proj else (thresh, border)


def stack_well_masks_batch(handle: Handle, stacks, out_hw, seed=0, warn=print):
    """--detect-well for n Z stacks of one shape: stack_well_masks of every stack, fallbacks and warnings included, with the pixel
    stages of all n in one launch set (stack_well_front) and the fit once per batch (make_well_masks_from_front).  stacks: as
    analyze_stack_batch takes them -> (well (n, fh, fw) bool, pruning (n, fh, fw) bool)"""
    from . import well_mask_generation as wmg
    thresh, border = stack_well_front(handle, stacks, out_hw)
    well, shrunken = wmg.make_well_masks_from_front(thresh, border, out_hw, handle, seed, warn)
    return well, np.logical_not(shrunken)


def stack_field(handle: Handle, stack: np.ndarray, ds_width=384, hessian="gaussian_derivatives") -> np.ndarray:
    """compute_branches.py:247-302 for one stack: the (round(H ds_width / W), ds_width) vesselness image"""
    a = _as_u16_stack(stack)
    out_hw = dsamp_shape(a.shape, ds_width)
    return vessel_field(handle, stack_prepare(handle, a, out_hw), hessian)
