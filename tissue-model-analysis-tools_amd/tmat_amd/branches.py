"""Batched analyze_img (reference scripts/compute_branches.py:144-489, 2-D branch) over the C-ABI."""
from __future__ import annotations

import ctypes as C
from itertools import product

import numpy as np

from . import _lib

DOWNSAMPLE_WIDTH = 384


def pixels_to_microns(num_pixels: float, im_width_px: int, im_width_microns: float) -> float:
    return (im_width_microns / im_width_px) * num_pixels


def microns_to_pixels(num_microns: float, im_width_px: int, im_width_microns: float) -> float:
    return (im_width_px / im_width_microns) * num_microns


def graph_px_params(config: dict, field_width: int, image_width_microns: float):
    """compute_branches.py:401-415"""
    min_px = round(microns_to_pixels(config.get("min_branch_length", 12), field_width, image_width_microns))
    mx = config.get("max_branch_length")
    max_px = None if mx is None else round(max(1, microns_to_pixels(mx, field_width, image_width_microns)))
    sw_px = round(max(1, microns_to_pixels(config.get("graph_smoothing_window", 12), field_width, image_width_microns)))
    return sw_px, min_px, max_px


def threshold_grid(config: dict):
    """compute_branches.py:366-395: Cartesian grid over graph_thresh_1 x graph_thresh_2 with the file-name suffix."""
    params = {"thresh1": np.atleast_1d(config.get("graph_thresh_1", 5)).tolist(),
              "thresh2": np.atleast_1d(config.get("graph_thresh_2", 10)).tolist()}
    names, vals = zip(*params.items())
    cfgs = [dict(zip(names, comb)) for comb in product(*vals)]
    tuned = [k for k, v in params.items() if len(v) > 1]
    fmts = {}
    for k, v in params.items():
        if all(isinstance(x, (int, float)) for x in v):
            if all(isinstance(x, int) for x in v):
                fmts[k] = f"{{:0{max(len(str(x)) for x in v)}d}}"
            else:
                wl = max(str(float(x)).find(".") for x in v)
                wr = max(len(str(float(x)).split(".")[1]) for x in v)
                fmts[k] = f"{{:0{wl + 1 + wr}.{wr}f}}"
        else:
            fmts[k] = "{}"
    out = []
    for cfg in cfgs:
        s = "".join(f"_{k}_{fmts[k].format(v)}" for k, v in cfg.items() if k in tuned)
        out.append((cfg, f"_CONFIG{s}" if s else ""))
    return out


# The marshalling the analyze_batch* functions share: every one of them describes its call with these and hands it to its own C entry.

def _shapes(H: int, W: int, ds_ratio: float):
    """((hh, ww), (fh, fw)) of (H, W) images: the network's input shape -- cv2 reads dsize as (width, height) -- and the field's"""
    return (int(round(W * ds_ratio)), int(round(H * ds_ratio))), dsamp_shape((H, W))


def _as_u8(m, shape, who: str, what: str):
    """a caller's masks (None passes through) as a contiguous 0 / 1 u8 array of `shape`"""
    if m is None:
        return None
    m = np.asarray(m)
    if m.shape != tuple(shape):
        raise ValueError(f"{who}: {what} have shape {m.shape}, expected {tuple(shape)}")
    return np.ascontiguousarray(m != 0, np.uint8)


def _graph_fields(config: dict, image_width_microns: float, first_index: int) -> dict:
    """the graph parameters in pixels and the first index, under tmat_analyze_opts' field names and in the positional entries' order"""
    sw_px, min_px, max_px = graph_px_params(config, DOWNSAMPLE_WIDTH, image_width_microns)
    return dict(smoothing_window_px=int(sw_px), min_branch_length_px=int(min_px), max_branch_length_px=int(max_px or 0),
                remove_isolated=int(bool(config.get("remove_isolated_branches", False))), first_index=int(first_index))


def _positional_args(shape, config: dict, image_width_microns: float, ds_ratio: float, thresh, first_index: int):
    """what tmat_analyze_batch, _masked and _tree take between the image pointer and their own outputs; shape = (n, H, W)"""
    return (*shape, float(ds_ratio), DOWNSAMPLE_WIDTH, float(thresh[0]), float(thresh[1]),
            *_graph_fields(config, image_width_microns, first_index).values())


def _analyze_opts(config: dict, image_width_microns: float, ds_ratio: float, first_index: int, thresh=(0.0, 0.0), well=None, pruning=None):
    """tmat_analyze_opts without requests; well / pruning: _as_u8's arrays, which the caller keeps alive"""
    return _lib.AnalyzeOpts(size=C.sizeof(_lib.AnalyzeOpts), ds_ratio=float(ds_ratio), ds_width=DOWNSAMPLE_WIDTH, graph_thresh_1=float(thresh[0]),
                            graph_thresh_2=float(thresh[1]), well_masks=None if well is None else well.ctypes.data,
                            pruning_masks=None if pruning is None else pruning.ctypes.data,
                            **_graph_fields(config, image_width_microns, first_index))


def _entry(handle: _lib.Handle, name: str, input_bits: int):
    """C entry point `name` bound to the handle, whose input depth is set first"""
    L = _lib.lib()
    _lib.check(L.tmat_set_input_depth(handle.raw, int(input_bits)), "tmat_set_input_depth")
    fn = getattr(L, name)
    return lambda *args: fn(handle.raw, *args)


def _retry_bars(lead_shape, cap_bars: int, full: int, call):
    """call(bars, cap) -> return code, with bars an empty (*lead_shape, cap, 2) f64 array.  A branch holds at least one vertex of its own,
    so `full` = fh * fw bars always suffice: one retry with that capacity when cap_bars is too small.  Returns (code, bars)."""
    for cap in (int(cap_bars), max(int(cap_bars), full)):
        bars = np.empty(tuple(lead_shape) + (cap, 2), np.float64)
        rc = call(bars, cap)
        if rc != _lib.E_CAP or cap >= full:
            break
    return rc, bars


def _row_tuples(rows):
    return [(r.index, r.count, r.total_px, r.avg_px) for r in rows]


def analyze_batch(handle: _lib.Handle, imgs: np.ndarray, config: dict, image_width_microns: float, ds_ratio: float = 0.625,
                  thresh=(5.0, 10.0), first_index: int = 0, dev_ptr=None, input_bits: int = 16):
    """imgs (n, H, W) uint16 (host) or a device pointer + shape -> list of (index, count, total_px, avg_px).
    `input_bits` = 8 for images that were uint8 before widening (cv2.resize saturates to the source depth)."""
    if dev_ptr is None:
        imgs = np.ascontiguousarray(imgs, np.uint16)
    shape = imgs.shape if dev_ptr is None else tuple(imgs)
    rows = (_lib.Row * shape[0])()
    name = "tmat_analyze_batch" if dev_ptr is None else "tmat_analyze_batch_dev"
    _lib.check(_entry(handle, name, input_bits)(_lib.ptr(imgs) if dev_ptr is None else C.c_void_p(dev_ptr),
                                                *_positional_args(shape, config, image_width_microns, ds_ratio, thresh, first_index), rows), name)
    return _row_tuples(rows)


def analyze_batch_tree(handle: _lib.Handle, imgs: np.ndarray, config: dict, image_width_microns: float, ds_ratio: float = 0.625,
                       thresh=(5.0, 10.0), first_index: int = 0, input_bits: int = 16, vis_width: int = 2000, cap_bars: int = 4096):
    """analyze_batch "with tree" (tmat_analyze_batch_tree): imgs (n, H, W) uint16 -> (rows as analyze_batch returns them, overlays
    (n, vh, vw, 3) u8 drawn per pass on the device over the down-sampled images, [bars (k, 2) f64 scaled] per image)."""
    imgs = np.ascontiguousarray(imgs, np.uint16)
    n, H, W = imgs.shape
    (hh, ww), (fh, fw) = _shapes(H, W, ds_ratio)
    rows = (_lib.Row * n)()
    rgb = np.empty((n,) + tuple(_lib.tree_canvas_shape(hh, ww, vis_width)) + (3,), np.uint8)
    nb = np.zeros(n, np.int32)
    fn = _entry(handle, "tmat_analyze_batch_tree", input_bits)
    args = _positional_args(imgs.shape, config, image_width_microns, ds_ratio, thresh, first_index)
    rc, bars = _retry_bars((n,), cap_bars, fh * fw, lambda bars, cap: fn(_lib.ptr(imgs), *args, rows, int(vis_width), _lib.ptr(rgb), _lib.ptr(bars),
                                                                          cap, _lib.ptr(nb)))
    _lib.check(rc, "tmat_analyze_batch_tree")
    return _row_tuples(rows), rgb, [bars[i, : nb[i]].copy() for i in range(n)]


def analyze_batch_ex(handle: _lib.Handle, imgs: np.ndarray, config: dict, image_width_microns: float, ds_ratio: float = 0.625,
                     thresh=(5.0, 10.0), first_index: int = 0, input_bits: int = 16, well_masks=None, pruning_masks=None, tree: bool = False,
                     vis_width: int = 2000, stage_pictures: bool = False, cap_bars: int = 4096):
    """One batched call with any combination of requests (tmat_analyze_batch_ex): the rows of analyze_batch / analyze_batch_masked /
    analyze_batch_tree, plus what was asked for.  well_masks (n, h, w), pruning_masks (n, fh, fw): as analyze_batch_masked.  tree: the
    overlays and bars of analyze_batch_tree (with masks: the pruned graph's tree over the unmasked down-sampled image).
    stage_pictures: the (n, 4, h, w) u8 pictures of the reference's four image dumps (compute_branches.py:315, 331, 347, 348), planes
    in _lib.STAGE_PLANES order, rendered inside the pass from its buffers in HBM.
    Returns (rows, extras) with extras a dict holding "overlays" and "bars" (tree) and "pictures" (stage_pictures)."""
    imgs = np.ascontiguousarray(imgs, np.uint16)
    n, H, W = imgs.shape
    (hh, ww), (fh, fw) = _shapes(H, W, ds_ratio)
    well = _as_u8(well_masks, (n, hh, ww), "analyze_batch_ex", "well_masks")
    pruning = _as_u8(pruning_masks, (n, fh, fw), "analyze_batch_ex", "pruning_masks")
    rows = (_lib.Row * n)()
    o = _analyze_opts(config, image_width_microns, ds_ratio, first_index, thresh, well, pruning)
    extras = {}
    if stage_pictures:
        extras["pictures"] = np.empty((n, 4, hh, ww), np.uint8)
        o.stage_out = extras["pictures"].ctypes.data
    nb = np.zeros(n, np.int32)
    if tree:
        vh, vw = _lib.tree_canvas_shape(hh, ww, vis_width)
        extras["overlays"] = np.empty((n, vh, vw, 3), np.uint8)
        o.vis_width, o.rgb_out, o.n_bars = int(vis_width), extras["overlays"].ctypes.data, nb.ctypes.data
    fn = _entry(handle, "tmat_analyze_batch_ex", input_bits)

    def call(bars, cap):
        if tree:
            o.bars_out, o.cap_b = bars.ctypes.data, cap
        return fn(_lib.ptr(imgs), n, H, W, C.byref(o), rows) if n else 0
    rc, bars = _retry_bars((n,), cap_bars, fh * fw, call) if tree else (call(None, 0), None)
    _lib.check(rc, "tmat_analyze_batch_ex")
    if tree:
        extras["bars"] = [bars[i, : nb[i]].copy() for i in range(n)]
    return _row_tuples(rows), extras


def grid_pairs(config: dict):
    """the (graph_thresh_1, graph_thresh_2) pairs of threshold_grid(config), in its order"""
    return [(cfg["thresh1"], cfg["thresh2"]) for cfg, _ in threshold_grid(config)]


def grid_images_per_call(n_thresh: int, bytes_per_picture: int, budget: int = 1 << 30) -> int:
    """Images one tmat_analyze_batch_grid call takes when every (pair, image) owns bytes_per_picture bytes of the caller's picture
    buffers: the largest count that keeps them under `budget`, at least one.  The 1 GiB default caps host memory; it is not tuned."""
    return max(1, int(budget) // max(1, int(n_thresh) * int(bytes_per_picture)))


def grid_picture_bytes(img_shape, ds_ratio: float, vis_width: int, raw: bool, tree_png: bool, barcode_png: bool) -> int:
    """bytes of the caller's picture buffers one (pair, image) of analyze_batch_grid owns, for (H, W) images: the raw overlay, the worst-case
    overlay file, the worst-case barcode file -- whichever are asked for"""
    H, W = img_shape
    vh, vw = _lib.tree_canvas_shape(int(round(W * ds_ratio)), int(round(H * ds_ratio)), vis_width)
    S = int(round(vis_width * 0.9))
    return (vh * vw * 3 if raw else 0) + (_lib.png_bound(vh, vw, 3) if tree_png else 0) + (_lib.png_bound(S, S, 3) if barcode_png else 0)


def analyze_batch_grid(handle: _lib.Handle, imgs: np.ndarray, config: dict, image_width_microns: float, ds_ratio: float = 0.625, pairs=None,
                       first_index: int = 0, input_bits: int = 16, well_masks=None, pruning_masks=None, tree: bool = False, vis_width: int = 2000,
                       stage_pictures: bool = False, tree_png: bool = False, barcode_png: bool = False, raw_overlays: bool = True,
                       cap_bars: int = 4096, budget: int = 1 << 30):
    """The threshold grid from ONE pass of the network (tmat_analyze_batch_grid): imgs (n, H, W) uint16 -- or (device pointer, (n, H, W))
    for images resident in a tmat_dev_alloc block, through tmat_analyze_batch_grid_dev -- pairs [(graph_thresh_1,
    graph_thresh_2)] (None: grid_pairs(config)) -> ({pair: rows as analyze_batch returns them at that pair}, extras).  The requests are
    analyze_batch_ex's; what depends on the pair comes back per pair:
      tree            extras["bars"] = {pair: [bars (k, 2) f64 per image]} and, with raw_overlays, extras["overlays"] = {pair: (n, vh, vw, 3) u8}
      tree_png        extras["tree_png"] = {pair: [PNG file (bytes) per image]}: the overlays encoded on the device, nothing raw crosses when
                      raw_overlays is False
      barcode_png     extras["barcode_png"] = {pair: [PNG file per image]}: rasterised and encoded on the device from that pair's bars
      stage_pictures  extras["pictures"] (n, 4, h, w) u8, once: they do not depend on the pair
    tree_png / barcode_png imply tree.  With pictures the images go through in chunks of grid_images_per_call, so that the picture buffers
    of one call stay under `budget` bytes."""
    resident = isinstance(imgs, tuple)          # (device pointer, (n, H, W)): uint16 images in a tmat_dev_alloc block, read in place
    if resident:
        dev_ptr, (n, H, W) = imgs[0], (int(v) for v in imgs[1])
        dev_base = dev_ptr.value if isinstance(dev_ptr, C.c_void_p) else int(dev_ptr)
    else:
        imgs = np.ascontiguousarray(imgs, np.uint16)
        n, H, W = imgs.shape
    pairs = grid_pairs(config) if pairs is None else [(p[0], p[1]) for p in pairs]
    T = len(pairs)
    if T < 1:
        raise ValueError("analyze_batch_grid: no threshold pair")
    tree = bool(tree or tree_png or barcode_png)
    raw = bool(tree and raw_overlays)
    (hh, ww), (fh, fw) = _shapes(H, W, ds_ratio)
    well = _as_u8(well_masks, (n, hh, ww), "analyze_batch_grid", "well_masks")
    pruning = _as_u8(pruning_masks, (n, fh, fw), "analyze_batch_grid", "pruning_masks")
    rows_by = {p: [] for p in pairs}
    extras = {}
    if tree:
        extras["bars"] = {p: [] for p in pairs}
    if raw:
        extras["overlays"] = {p: [] for p in pairs}
    if tree_png:
        extras["tree_png"] = {p: [] for p in pairs}
    if barcode_png:
        extras["barcode_png"] = {p: [] for p in pairs}
    pics = []
    if n == 0:
        if raw:
            vh, vw = _lib.tree_canvas_shape(hh, ww, vis_width)
            extras["overlays"] = {p: np.empty((0, vh, vw, 3), np.uint8) for p in pairs}
        if stage_pictures:
            extras["pictures"] = np.empty((0, 4, hh, ww), np.uint8)
        return rows_by, extras
    thresh = np.ascontiguousarray(np.asarray(pairs, np.float32).reshape(T, 2))
    fn = _entry(handle, "tmat_analyze_batch_grid_dev" if resident else "tmat_analyze_batch_grid", input_bits)
    vh = vw = S = tcap = bcap = 0
    if tree:
        vh, vw = _lib.tree_canvas_shape(hh, ww, vis_width)
        S = int(round(vis_width * 0.9))
        tcap = _lib.png_bound(vh, vw, 3) if tree_png else 0
        bcap = _lib.png_bound(S, S, 3) if barcode_png else 0
    per_picture = (vh * vw * 3 if raw else 0) + tcap + bcap
    step = grid_images_per_call(T, per_picture, budget) if per_picture else n
    for i0 in range(0, n, step):
        k = min(step, n - i0)
        rows = (_lib.Row * (T * k))()
        o = _analyze_opts(config, image_width_microns, ds_ratio, int(first_index) + i0, well=None if well is None else well[i0:],
                          pruning=None if pruning is None else pruning[i0:])
        g = _lib.GridOpts(size=C.sizeof(_lib.GridOpts), n_thresh=T, thresh=thresh.ctypes.data)
        if stage_pictures:
            pics.append(np.empty((k, 4, hh, ww), np.uint8))
            o.stage_out = pics[-1].ctypes.data
        nb = np.zeros((T, k), np.int32)
        if tree:
            o.vis_width, o.n_bars = int(vis_width), nb.ctypes.data
            if raw:
                rgb = np.empty((T, k, vh, vw, 3), np.uint8)
                o.rgb_out = rgb.ctypes.data
            if tree_png:
                tfiles, tsizes = np.empty((T, k, tcap), np.uint8), np.zeros((T, k), np.uintp)
                g.tree_png, g.tree_png_cap, g.tree_png_sizes = tfiles.ctypes.data, tcap, tsizes.ctypes.data
            if barcode_png:
                bfiles, bsizes = np.empty((T, k, bcap), np.uint8), np.zeros((T, k), np.uintp)
                g.barcode_png, g.barcode_png_cap, g.barcode_png_sizes = bfiles.ctypes.data, bcap, bsizes.ctypes.data

        def call(bars, cap):
            if tree:
                o.bars_out, o.cap_b = bars.ctypes.data, cap
            src = C.c_void_p(dev_base + i0 * H * W * 2) if resident else _lib.ptr(imgs[i0:])
            return fn(src, k, H, W, C.byref(o), C.byref(g), rows)
        rc, bars = _retry_bars((T, k), cap_bars, fh * fw, call) if tree else (call(None, 0), None)
        _lib.check(rc, "tmat_analyze_batch_grid")
        for t, p in enumerate(pairs):
            rows_by[p] += _row_tuples(rows[t * k:(t + 1) * k])
            if tree:
                extras["bars"][p] += [bars[t, i, : nb[t, i]].copy() for i in range(k)]
            if raw:
                extras["overlays"][p].append(rgb[t])
            if tree_png:
                extras["tree_png"][p] += [tfiles[t, i, : int(tsizes[t, i])].tobytes() for i in range(k)]
            if barcode_png:
                extras["barcode_png"][p] += [bfiles[t, i, : int(bsizes[t, i])].tobytes() for i in range(k)]
    if raw:
        extras["overlays"] = {p: np.concatenate(v) for p, v in extras["overlays"].items()}
    if stage_pictures:
        extras["pictures"] = np.concatenate(pics)
    return rows_by, extras


def _unique_path(vis_dir, name):
    """vis_dir / name under the reference's "-N" unique-name rule (helper.get_unique_output_filepath); makes vis_dir"""
    import os
    from pathlib import Path
    vis_dir = Path(vis_dir)
    vis_dir.mkdir(parents=True, exist_ok=True)
    file = vis_dir / name
    stem, ext = os.path.splitext(file.name)
    n = 1
    while file.exists():
        n += 1
        file = vis_dir / f"{stem}-{n}{ext}"
    return file


def write_png_batch(items, encoder):
    """items: [(picture, vis_dir, name)], a picture being an (h, w) / (h, w, 3) u8 array or a finished PNG file (bytes).  All arrays of
    one shape are encoded in ONE call of encoder ((n, h, w[, 3]) u8 -> n files: _lib.Handle.png_encode, _lib.host_png_encode); the
    files are then written in the order given, each under the "-N" unique-name rule.  Returns the written paths."""
    groups = {}
    for k, (a, _, _) in enumerate(items):
        if not isinstance(a, (bytes, bytearray)):
            a = np.ascontiguousarray(a, np.uint8)
            groups.setdefault(a.shape, []).append((k, a))
    data = {k: a for k, (a, _, _) in enumerate(items) if isinstance(a, (bytes, bytearray))}
    for members in groups.values():
        files = encoder(np.stack([a for _, a in members]))
        data.update({k: f for (k, _), f in zip(members, files)})
    out = []
    for k, (_, vis_dir, name) in enumerate(items):
        file = _unique_path(vis_dir, name)
        file.write_bytes(data[k])
        out.append(str(file))
    return out


def _save_png_unique(a, vis_dir, name, encoder=None):
    """a finished u8 picture into vis_dir / name under the reference's "-N" unique-name rule (helper.get_unique_output_filepath).
    encoder None: PIL; else the file comes from encoder (write_png_batch)"""
    if encoder is not None:
        return write_png_batch([(a, vis_dir, name)], encoder)[0]
    from PIL import Image
    file = _unique_path(vis_dir, name)
    Image.fromarray(np.ascontiguousarray(a, np.uint8)).save(file)
    return str(file)


STAGE_PICTURE_FILES = ("original_image.png", "prediction.png", "segmentation_mask.png", "distance_transform.png")


def stage_picture_items(pictures, vis_dir, well_mask=None):
    """write_png_batch's items of one image's (4, h, w) stage pictures (+ well_mask.png)"""
    pictures = np.asarray(pictures)
    if pictures.ndim != 3 or pictures.shape[0] != 4:
        raise ValueError(f"save_stage_pictures: expected (4, h, w) pictures, got {pictures.shape}")
    items = [(pictures[k], vis_dir, name) for k, name in enumerate(STAGE_PICTURE_FILES)]
    if well_mask is not None:
        items.append((_lib.host_stage_pictures((np.asarray(well_mask) != 0).astype(np.uint8) * 255), vis_dir, "well_mask.png"))
    return items


def save_stage_pictures(pictures, vis_dir, well_mask=None, encoder=None):
    """One image's (4, h, w) u8 stage pictures (analyze_batch_ex(stage_pictures=True)["pictures"][i]) as the reference's four files
    (compute_branches.py:315, 331, 347, 348), and with well_mask (h, w) also well_mask.png = save_vis(well_mask * 255) (:364).
    Names follow the "-N" unique-name rule.  encoder (write_png_batch) None: PIL, file by file; else one encoder call for the image's
    pictures (a batch of images in one call: stage_picture_items + write_png_batch).  Returns the written paths."""
    items = stage_picture_items(pictures, vis_dir, well_mask)
    if encoder is not None:
        return write_png_batch(items, encoder)
    return [_save_png_unique(a, d, name) for a, d, name in items]


def tree_picture_items(overlay, bars, vis_dir, suffix: str = "", vis_width: int = 2000):
    """write_png_batch's items of one image's morse_tree / barcode pair (overlay: the raster, or its finished PNG file); none without branches"""
    if len(bars) == 0:
        return []
    return [(overlay, vis_dir, f"morse_tree{suffix}.png"), (_lib.host_render_barcode(bars, vis_width), vis_dir, f"barcode{suffix}.png")]


def save_tree_pictures(overlay, bars, vis_dir, suffix: str = "", vis_width: int = 2000, encoder=None):
    """morse_tree{suffix}.png (a finished overlay) and barcode{suffix}.png into vis_dir, "-N" unique names; nothing for an image without
    branches (the reference prints "No branches found" and skips its plots, compute_branches.py:426-429).  encoder (write_png_batch)
    None: PIL; with it the overlay may also be a finished PNG file (Handle.render_tree_png).  Returns the written paths."""
    items = tree_picture_items(overlay, bars, vis_dir, suffix, vis_width)
    if encoder is not None:
        return write_png_batch(items, encoder)
    from PIL import Image
    out = []
    for a, d, name in items:
        file = _unique_path(d, name)
        Image.fromarray(np.ascontiguousarray(a), "RGB").save(file)
        out.append(str(file))
    return out


def dsamp_shape(img_shape, width: int = DOWNSAMPLE_WIDTH):
    """compute_branches.py:218-222: img_dsamp_res = round(shape * width / W)"""
    r = width / img_shape[1]
    return tuple(int(v) for v in np.round(np.multiply(img_shape[:2], r)).astype(int))


def well_fields(handle: _lib.Handle, imgs: np.ndarray, ds_ratio: float = 0.625, input_bits: int = 16, well_seed: int = 0, warn=print,
                return_backgrounds: bool = False):
    """The 2-D branch of analyze_img with use_well_mask=True up to the vesselness field (compute_branches.py:309-361), image by
    image through the staged GPU entry points: Lanczos + rescale (tmat_preprocess_batch) -> make_well_mask on THAT image
    (:318-319, tmat_amd/well_mask_generation.py) -> predict(img * well_mask) (:328) -> (pred > 0.5) * well_mask ->
    filter_branch_seg_mask (:334-337) -> medial axis, centre-line weighting of the unmasked prediction, resize (:340-357).
    Returns [(field255 (fh, fw) f32, pruning_mask (fh, fw) bool, well_mask)] per image: the graph stages follow per threshold.
    return_backgrounds: also return the (n, hh, ww) f32 down-sampled images (:312-314 original_image, min-max rescaled to 0..1: the tree
    overlay rescales its background itself, so the grey levels are those of the Lanczos image)."""
    from . import well_mask_generation as wmg
    imgs = np.ascontiguousarray(imgs, np.uint16)
    n, H, W = imgs.shape
    hh, ww = int(round(W * ds_ratio)), int(round(H * ds_ratio))            # cv2 reads dsize as (width, height)
    L = _lib.lib()
    x = np.empty((n, hh, ww), np.float32)
    _lib.check(L.tmat_set_input_depth(handle.raw, int(input_bits)), "tmat_set_input_depth")
    _lib.check(L.tmat_preprocess_batch(handle.raw, _lib.ptr(imgs), n, H, W, float(ds_ratio), _lib.ptr(x)), "tmat_preprocess_batch")
    _lib.check(L.tmat_set_input_depth(handle.raw, 16), "tmat_set_input_depth")
    masks = [wmg.make_well_mask(x[i], handle=handle, seed=well_seed, warn=warn) for i in range(n)]
    well = np.stack([m[0] for m in masks])
    pred = handle.predict_smooth(x * well)                                  # img * well_mask: float32 * bool
    filt = handle.filter_mask((pred > 0.5) & well)                          # seg_mask * well_mask, footprint disk(2), remove_isolated
    skel, dist = handle.medial_axis(filt)
    # the reference resizes to img_dsamp_res computed from the ORIGINAL image shape (:218-222)
    fshape = dsamp_shape((H, W))
    _, f255 = handle.finish(pred, dist, skel, fshape)
    out = []
    for i in range(n):
        pruning = wmg._resize_nearest(np.logical_not(masks[i][1]), fshape).astype(bool)      # resize(order=0) (:359-361)
        out.append((f255[i], pruning, well[i]))
    return (out, x) if return_backgrounds else out


def well_rows(handle: _lib.Handle, fields, config: dict, image_width_microns: float, thresh=(5.0, 10.0), first_index: int = 0):
    """graph stages of the --detect-well form (compute_branches.py:391-457): DMT graph of the 0..255 field, MorseGraph with the
    pruning mask -> rows (index, count, total_px, avg_px)"""
    rows = []
    for i, (f255, pruning, _) in enumerate(fields):
        sw_px, min_px, max_px = graph_px_params(config, f255.shape[1], image_width_microns)
        V, E = _lib.dmt_graph(f255, thresh[0], thresh[1], handle=handle)
        _, cnt, tot, avg = _lib.morse_stats(V, E, f255.shape, sw_px, min_px, max_px, bool(config.get("remove_isolated_branches", False)),
                                            pruning)
        rows.append((first_index + i, cnt, tot, avg))
    return rows


def analyze_batch_masked(handle: _lib.Handle, imgs: np.ndarray, config: dict, image_width_microns: float, ds_ratio: float = 0.625,
                         thresh=(5.0, 10.0), first_index: int = 0, input_bits: int = 16, well_masks=None, pruning_masks=None):
    """analyze_batch with well masks (tmat_analyze_batch_masked): well_masks (n, h, w) over the down-sampled images, (h, w) =
    (round(W ds_ratio), round(H ds_ratio)), multiply the network input and the thresholded mask; pruning_masks (n, fh, fw) over the
    fields, (fh, fw) = dsamp_shape((H, W)), prune the graphs.  Either may be None; with both None the rows are analyze_batch's."""
    imgs = np.ascontiguousarray(imgs, np.uint16)
    n, H, W = imgs.shape
    (hh, ww), (fh, fw) = _shapes(H, W, ds_ratio)
    well = _as_u8(well_masks, (n, hh, ww), "analyze_batch_masked", "well_masks")
    pruning = _as_u8(pruning_masks, (n, fh, fw), "analyze_batch_masked", "pruning_masks")
    rows = (_lib.Row * n)()
    _lib.check(_entry(handle, "tmat_analyze_batch_masked", input_bits)(
        _lib.ptr(imgs), *_positional_args(imgs.shape, config, image_width_microns, ds_ratio, thresh, first_index),
        None if well is None else _lib.ptr(well), None if pruning is None else _lib.ptr(pruning), rows), "tmat_analyze_batch_masked")
    return _row_tuples(rows)


def analyze_batch_well(handle: _lib.Handle, imgs: np.ndarray, config: dict, image_width_microns: float, ds_ratio: float = 0.625,
                       thresh=(5.0, 10.0), first_index: int = 0, input_bits: int = 16, well_seed: int = 0, warn=print, masks=None,
                       stage_pictures: bool = False, pairs=None):
    """The --detect-well form of the 2-D branch through the batch pipeline: the rows of well_fields + well_rows.  Lanczos + rescale
    (tmat_preprocess_batch) -> make_well_masks_batch on those images (the superellipse fit of the whole batch on the device) ->
    pruning masks = resize(~shrunken, field shape, order 0) (compute_branches.py:359-361) -> tmat_analyze_batch_masked, which repeats
    the Lanczos pass inside its pipeline.  masks: a (well, pruning) pair from an earlier call on the same images (the masks do not depend
    on the graph thresholds).  Returns (rows, well (n, h, w) bool, pruning (n, fh, fw) bool); with stage_pictures also the (n, 4, h, w) u8
    pictures of analyze_batch_ex, out of the same call.  pairs (a list of (graph_thresh_1, graph_thresh_2); thresh is then not read): the
    whole grid from one masked pass (analyze_batch_grid) -- rows is then {pair: rows}."""
    from . import well_mask_generation as wmg
    imgs = np.ascontiguousarray(imgs, np.uint16)
    n, H, W = imgs.shape
    if masks is None:
        hh, ww = int(round(W * ds_ratio)), int(round(H * ds_ratio))        # cv2 reads dsize as (width, height)
        L = _lib.lib()
        x = np.empty((n, hh, ww), np.float32)
        _lib.check(L.tmat_set_input_depth(handle.raw, int(input_bits)), "tmat_set_input_depth")
        _lib.check(L.tmat_preprocess_batch(handle.raw, _lib.ptr(imgs), n, H, W, float(ds_ratio), _lib.ptr(x)), "tmat_preprocess_batch")
        well, shrunken = wmg.make_well_masks_batch(x, handle, seed=well_seed, warn=warn)
        fshape = dsamp_shape((H, W))
        pruning = np.stack([wmg._resize_nearest(np.logical_not(shrunken[i]), fshape) for i in range(n)]).astype(bool)
    else:
        well, pruning = masks
    if pairs is not None:
        rows, extras = analyze_batch_grid(handle, imgs, config, image_width_microns, ds_ratio, pairs, first_index, input_bits, well, pruning,
                                          stage_pictures=stage_pictures)
        return (rows, well, pruning, extras["pictures"]) if stage_pictures else (rows, well, pruning)
    if stage_pictures:
        rows, extras = analyze_batch_ex(handle, imgs, config, image_width_microns, ds_ratio, thresh, first_index, input_bits, well, pruning,
                                        stage_pictures=True)
        return rows, well, pruning, extras["pictures"]
    rows = analyze_batch_masked(handle, imgs, config, image_width_microns, ds_ratio, thresh, first_index, input_bits, well, pruning)
    return rows, well, pruning


def field_tree(handle, field255: np.ndarray, config: dict, image_width_microns: float, thresh=(5.0, 10.0), pruning_mask=None,
               scaling_factor: float = 1.0):
    """The colored tree of one 0..255 field (compute_branches.py:401-426 + topology.py:358-389): DMT graph, MorseGraph with the pruning mask
    -> ((segs, seg_branch), bars scaled, (count, total_px, avg_px)) through tmat_morse_tree.  The --detect-well and Z-stack forms of
    --tree-visualizations draw this over their own backgrounds (save_tree_visualizations)."""
    sw_px, min_px, max_px = graph_px_params(config, field255.shape[1], image_width_microns)
    V, E = _lib.dmt_graph(field255, thresh[0], thresh[1], handle=handle)
    segs, sb, bars, cnt, tot, avg = _lib.morse_tree(V, E, field255.shape, sw_px, min_px, max_px, bool(config.get("remove_isolated_branches", False)),
                                                    pruning_mask, scaling_factor)
    return (segs, sb), bars, (cnt, tot, avg)


class InputError(Exception):
    """an image of the run cannot be loaded / lacks its physical width: raised by run_sharded's callbacks (after they have
    printed the reference's message); the run then fails on EVERY rank after the gather instead of leaving the others blocked"""


def run_sharded(ids, load_fn, width_fn, analyze_fn, config: dict, rank: int = 0, world_size: int = 1, chunk: int = 64,
                log=print, pass_ids: bool = False, chunk_ends=None, stack_fn=None):
    """The per-run driver of scripts/compute_branches.py (reference :585-594 loops over the images one by one):
    rank `rank` of `world_size` takes a contiguous block of `ids`, loads its images in bounded chunks of at most `chunk`
    (images of equal shape, physical width and bit depth are analysed as one batch), and all ranks exchange their rows
    with one all-gather per threshold configuration.

    load_fn(img_id) -> uint8/uint16 (H, W) array; width_fn(img_id, img) -> image width in microns;
    analyze_fn(batch uint16 (n, H, W), width_um, thresh=(t1, t2), input_bits=8|16) -> [(i, count, total_px, avg_px)].
    pass_ids: analyze_fn also takes ids=[the id of every image of the batch, in batch order] (the pictures of --tree-visualizations
    are written per image inside analyze_fn).
    chunk_ends (optional): chunk_ends(keys of the images held, key of the next image, next image) -> bool, asked before an image joins
    the held chunk; True analyses the held chunk first (the Z-stack path groups consecutive stacks of one key under a byte budget).
    stack_fn (optional): stack_fn([what load_fn returned for the images of one group]) -> the batch handed to analyze_fn in place of
    np.stack(...).astype(np.uint16); load_fn may then return any object with shape and dtype (helper.PlaneSource: files not yet decoded,
    the group is decoded in flush).  A batch with a free() method is freed when its group is done.
    Returns {file-name suffix: [(global index, count, total_um, avg_um)] sorted by index}, on every rank."""
    from . import distributed
    ids = list(ids)
    grid = threshold_grid(config)
    results = {suffix: [] for _, suffix in grid}
    mine = distributed.shard_indices(len(ids), rank, world_size)

    def flush(groups):
        for (shape, width_um, bits), items in groups.items():
            batch = stack_fn([im for _, im in items]) if stack_fn is not None else np.stack([im for _, im in items]).astype(np.uint16)
            extra = {"ids": [ids[g] for g, _ in items]} if pass_ids else {}
            try:
                for cfg, suffix in grid:
                    rows = analyze_fn(batch, width_um, thresh=(cfg["thresh1"], cfg["thresh2"]), input_bits=bits, **extra)
                    for (gidx, _), r in zip(items, rows):
                        results[suffix].append((gidx, r[1], pixels_to_microns(r[2], DOWNSAMPLE_WIDTH, width_um),
                                                pixels_to_microns(r[3], DOWNSAMPLE_WIDTH, width_um)))
            finally:
                if hasattr(batch, "free"):
                    batch.free()

    # Whatever goes wrong on this rank -- an unreadable image (InputError), a HIP / library error out of analyze_fn, a shape
    # surprise in np.stack -- the rank must still enter the collective below: the other ranks are waiting in it and would block
    # until the launcher kills them.  The failure travels through the gather (distributed.gather_rows raises RankFailed everywhere).
    groups, held, failed, held_keys = {}, 0, False, []
    try:
        for gidx in mine:
            img_id = ids[int(gidx)]
            log(f"Analyzing {img_id}...")
            try:
                img = load_fn(img_id)
                width_um = width_fn(img_id, img)
            except InputError:
                failed = True
                break
            key = (img.shape, float(width_um), 8 * img.dtype.itemsize)
            if chunk_ends is not None and held and chunk_ends(held_keys, key, img):
                flush(groups)
                groups, held, held_keys = {}, 0, []
            groups.setdefault(key, []).append((int(gidx), img))
            held += 1
            held_keys.append(key)
            if held >= chunk:           # bounded host / HBM footprint: the reference streams one image at a time
                flush(groups)
                groups, held, held_keys = {}, 0, []
        if not failed:
            flush(groups)
    except Exception:                   # noqa: BLE001 -- reported here, re-raised as RankFailed by the gather on every rank
        import traceback
        traceback.print_exc()
        log(f"rank {rank}: the shard failed (traceback above); entering the gather with the failure marker")
        failed = True
    return {suffix: distributed.gather_rows(results[suffix], n_total=len(ids), failed=failed) for _, suffix in grid}


def stage_pictures_staged(handle: _lib.Handle, img: np.ndarray, ds_ratio: float = 0.625, input_bits: int = 16):
    """The four stage pictures of one image the staged way, without the batch pipeline: segment -> filter + EDT -> host medial axis, the
    centre-line weighting of compute_branches.py:341-344 with the scipy call the reference makes, a host Lanczos for the original, and
    save_vis (:74-78) in numpy.  Returns [original, prediction, mask, weighted] u8 (h, w) arrays; writes no file.  This is what
    save_visualizations has always computed, and the independent reference of analyze_batch_ex(stage_pictures=True)."""
    from scipy.ndimage import distance_transform_edt

    img = np.ascontiguousarray(img, np.uint16)
    H, W = img.shape
    hh, ww = int(round(W * ds_ratio)), int(round(H * ds_ratio))            # cv2 reads dsize as (width, height)
    L = _lib.lib()
    pred = np.empty((1, hh, ww), np.float64)
    _lib.check(L.tmat_set_input_depth(handle.raw, int(input_bits)), "tmat_set_input_depth")
    _lib.check(L.tmat_segment_batch(handle.raw, _lib.ptr(img[None]), 1, H, W, float(ds_ratio), _lib.ptr(pred)), "tmat_segment_batch")
    _lib.check(L.tmat_set_input_depth(handle.raw, 16), "tmat_set_input_depth")
    filt, dist = handle.filter_edt(pred)
    skel, _ = _lib.host_medial_axis(filt[0])
    cdt = distance_transform_edt(np.logical_not(skel))
    with np.errstate(invalid="ignore", divide="ignore"):
        weighted = pred[0] * (dist[0] / (dist[0] + cdt))
    original = _lib.host_lanczos4_u16(img, (hh, ww))        # uint8 sources: float path, a 1-LSB-level difference in a picture
    return [save_vis_u8(original), save_vis_u8(pred[0]), save_vis_u8(filt[0].astype(np.float64)), save_vis_u8(weighted)]


def save_vis_u8(a):
    """save_vis's arithmetic (compute_branches.py:74-78: rescale_intensity to 0..255 and cv2.imwrite's cast) in numpy -> u8"""
    import warnings
    a = np.asarray(a, np.float64)
    with warnings.catch_warnings(), np.errstate(invalid="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)         # an all-NaN image
        lo, hi = np.nanmin(a), np.nanmax(a)
        a = np.clip(a, lo, hi)
        a = (a - lo) / (hi - lo) * 255.0 if hi != lo else np.clip(a, 0, 255)
    return np.rint(np.nan_to_num(a)).astype(np.uint8)


def save_visualizations(handle: _lib.Handle, img: np.ndarray, vis_dir, ds_ratio: float = 0.625, input_bits: int = 16, encoder=None):
    """The four image dumps of the reference's 2-D branch (compute_branches.py:74-78 save_vis = rescale_intensity to
    0..255 + cv2.imwrite; :315 original_image.png, :331 prediction.png, :347 segmentation_mask.png, :348
    distance_transform.png) for one image, through the staged entry points of the same GPU path (stage_pictures_staged: a second
    pass over the image beside the batch pipeline; analyze_batch_ex(stage_pictures=True) + save_stage_pictures take them out of the
    pipeline's own pass).  The barcode / tree pictures (:431-450) are save_tree_visualizations' job.  encoder: write_png_batch's (None:
    PIL).  Returns the written paths."""
    return save_stage_pictures(np.stack(stage_pictures_staged(handle, img, ds_ratio, input_bits)), vis_dir, encoder=encoder)


def save_stack_visualizations(handle: _lib.Handle, stack: np.ndarray, vis_dir, hessian: str = "gaussian_derivatives", encoder=None):
    """The two image dumps of the reference's Z-stack branch (compute_branches.py:228-229 original_image.png = the max
    projection, :303 vesselness_image.png) for one stack, through the same GPU path.  encoder: write_png_batch's (None: PIL).
    Returns the written paths."""
    from . import sato

    field = sato.stack_field(handle, stack, DOWNSAMPLE_WIDTH, hessian)

    def save_vis(a, name):
        a = np.asarray(a, np.float64)
        lo, hi = a.min(), a.max()
        a = (a - lo) / (hi - lo) * 255.0 if hi != lo else np.clip(a, 0, 255)
        return _save_png_unique(np.rint(a).astype(np.uint8), vis_dir, name, encoder)
    return [save_vis(np.asarray(stack).max(0), "original_image.png"), save_vis(field, "vesselness_image.png")]


def save_tree_visualizations(handle, background: np.ndarray, tree, bars, vis_dir, suffix: str = "", vis_width: int = 2000, encoder=None):
    """morse_tree{suffix}.png and barcode{suffix}.png of one image (compute_branches.py:431-450) as the library's rasters (DESIGN.md
    "Tree overlay and barcode pictures"), PNG-encoded with PIL.  background: the (bh, bw) u16 / f32 image the tree is drawn over; tree:
    (segs, seg_branch) and bars as _lib.morse_tree returns them, in background pixels; suffix: threshold_grid's "_CONFIG..." string.
    handle: the _lib.Handle whose device rasterises the overlay (tmat_render_tree); None asks for the host twin (tmat_host_render_tree, the
    same bytes).  Names follow the reference's "-N" unique-name rule.  An image without branches (the reference prints "No branches
    found" and skips its plots) writes nothing.  encoder (write_png_batch) None: PIL; with it and a handle the overlay is rendered and
    encoded back to back on the device (tmat_render_tree_png: only file bytes come back) and the barcode goes through encoder.
    Returns the written paths."""
    if len(bars) == 0:
        return []
    if encoder is not None and handle is not None:
        overlay = handle.render_tree_png(np.asarray(background)[None], [tree], vis_width)[0]
    else:
        render = handle.render_tree if handle is not None else _lib.host_render_tree
        overlay = render(np.asarray(background)[None], [tree], vis_width)[0]
    return save_tree_pictures(overlay, bars, vis_dir, suffix, vis_width, encoder)
