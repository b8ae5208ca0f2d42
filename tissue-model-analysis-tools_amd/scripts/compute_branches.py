#!/usr/bin/env python3
"""Analyze microvessels in a directory of 2-D Z-projections or of Z stacks -- MI355X drop-in for the reference's
scripts/compute_branches.py: same positional arguments, flags, config keys, CSV (utf-16, same header), config.json and
exit behaviour (message + exit code 1).  Projections go through the segmentation model (the 2-D branch,
compute_branches.py:307-361); Z stacks (slice sequences with a z<number> token, or multi-page files) through the Sato
branch (:224-306), both on the GPU.

    python compute_branches.py IN_ROOT OUT_ROOT [--image-width-microns F] [--graph-thresh-1 F ...]
        [--graph-thresh-2 F ...] [--min-branch-length F] [--max-branch-length F]
        [--remove-isolated-branches] [--graph-smoothing-window F] [-c CONFIG] [--channel N] [--time N] [-w]

Differences (documented in INTEGRATION.md): images are analysed in batches on the GPU (one process
per GPU under torch.distributed.run; rows are gathered over RCCL and rank 0 writes the CSV);
--detect-well takes an explicit --well-seed (the reference's random search is unseeded); the PNG image dumps are opt-in (--visualizations:
rendered on the GPU inside the batched analysis;
--tree-visualizations [--vis-width N] for the Morse tree and barcode pictures, which are the library's own rasters, not matplotlib's);
--sato-hessian picks the Hessian of skimage.filters.sato (gaussian_derivatives = scikit-image >= 0.20, what the reference's pinned 0.22.0 runs; gradient = <= 0.19);
without --image-width-microns (or the config key) the width comes from OME / ImageJ TIFF metadata
(tmat_amd/helper.py), as in the reference.
"""
import argparse
import contextlib
import csv
import ctypes as C
import json
import os
import sys
from glob import glob
from pathlib import Path

PKG = Path(__file__).resolve().parents[1]
if str(PKG) not in sys.path:
    sys.path.insert(0, str(PKG))

import numpy as np  # noqa: E402

DEFAULT_CONFIG_PATH = str(PKG / "config" / "default_branching_computation.json")
DOWNSAMPLE_WIDTH = 384
STACK_BATCH_DEFAULT = "1"          # TMAT_STACK_BATCH when unset: Z stacks of one shape go through tmat_analyze_stack_batch
FAIL = "\033[91m[FAILURE]\033[0m"
OK = "\033[92m[SUCCESS]\033[0m"


def parse_branching_args(arg_defaults):
    """same surface as the reference's script_util.parse_branching_args (script_util.py:40-204)"""
    p = argparse.ArgumentParser()
    p.add_argument("in_root", type=str)
    p.add_argument("out_root", type=str)
    p.add_argument("--channel", type=int, default=None)
    p.add_argument("--time", type=int, default=None)
    p.add_argument("-w", "--detect-well", action="store_true")
    p.add_argument("--well-seed", type=int, default=0,
                   help="seed of the random superellipse search of --detect-well (the reference draws from numpy's global, unseeded "
                        "generator: well_mask_generation.py:35; a run here equals a reference run after numpy.random.seed(SEED))")
    p.add_argument("--image-width-microns", type=float, default=None)
    p.add_argument("--graph-thresh-1", nargs="+", type=float, default=None)
    p.add_argument("--graph-thresh-2", nargs="+", type=float, default=None)
    p.add_argument("--min-branch-length", type=float, default=None)
    p.add_argument("--max-branch-length", type=float, default=None)
    p.add_argument("--remove-isolated-branches", action="store_true")
    p.add_argument("--graph-smoothing-window", type=float, default=None)
    p.add_argument("-c", "--config", type=str, default=arg_defaults["default_config_path"])
    p.add_argument("--tree-visualizations", action="store_true",
                   help="also write visualizations/<image>/{morse_tree,barcode}<_CONFIG...>.png per threshold configuration: the fitted branch "
                        "tree over the down-sampled image (Z stacks: over the full-resolution max projection) and the barcode; drawn on the GPU, for "
                        "2-D images inside the batched analysis")
    p.add_argument("--vis-width", type=int, default=2000, help="width in pixels of the morse_tree picture (default 2000)")
    p.add_argument("--visualizations", action="store_true",
                   help="also write visualizations/<image>/{original_image,prediction,segmentation_mask,distance_transform}.png "
                        "(Z stacks: {original_image,vesselness_image}.png; with -w also well_mask.png).  The reference always does; here it is "
                        "opt-in.  The pictures are rendered on the GPU from the arrays the batched analysis already holds, in the same pass")
    p.add_argument("--png-encoder", choices=["pil", "device"], default="pil",
                   help="who encodes the PNG pictures of --visualizations / --tree-visualizations: pil (the default: Pillow on the host, one "
                        "file after the other) or device (the library's deflate / PNG kernels: all pictures of one shape of a pass in one "
                        "batched call, only file bytes cross to the host).  The pixels are the same; the files differ in size")
    p.add_argument("--tiff-decoder", choices=["pil", "device"], default="pil",
                   help="Where TIFF pixels are decoded: pil (default; Pillow on the host, then an upload of raw pixels) or device (only the "
                        "file bytes are uploaded, the strips are decoded on the GPU and the batch routes read them where they land; files "
                        "the device path does not take still go through Pillow). The rows and pictures are the same.")
    p.add_argument("--png-compression", choices=["fast", "compact"], default="fast",
                   help="with --png-encoder device: fast (the default: fixed Huffman blocks) or compact (lazy matching and dynamic Huffman "
                        "blocks: smaller files for more time on the device).  The pixels are the same")
    p.add_argument("--sato-hessian", choices=["gaussian_derivatives", "gradient"], default="gaussian_derivatives",
                   help="Z stacks: Hessian of skimage.filters.sato -- gaussian_derivatives (scikit-image >= 0.20, the reference's pinned "
                        "0.22.0) or gradient (scikit-image <= 0.19)")
    args = p.parse_args()
    if not args.remove_isolated_branches:
        args.remove_isolated_branches = None
    for k, v in vars(args).items():
        if isinstance(v, str):
            setattr(args, k, v.strip("'\""))
    return args


def get_unique_output_filepath(file):
    file = Path(file)
    name, ext = os.path.splitext(file.name)
    n = 1
    while file.exists():
        n += 1
        file = file.parent / f"{name}-{n}{ext}"
    return file


def create_output_csv(output_file: Path):
    fields = ["Image", "Total # of branches", "Total branch length (µm)", "Average branch length (µm)"]
    with open(output_file, "w", encoding="utf-16") as f:
        csv.writer(f, lineterminator="\n").writerow(fields)


def load_image_2d(path: str, channel=None, time=None) -> np.ndarray:
    """One 2-D plane of an image file (reference helper.load_image :23-95 returns ZYX / YX for the chosen T and C; a time
    series needs --time, a multi-channel file --channel, as there).  .npy arrays: (H, W), or (C, H, W) / (H, W, C) with C <= 4."""
    from tmat_amd import helper
    if path.endswith(".npy"):
        a = np.load(path)
        if time not in (None, 0):
            raise ValueError(f"Time {time} is out of range for {path} with times: 0 - 0")
        if a.ndim == 3:
            cax = [ax for ax in (2, 0) if a.shape[ax] <= 4]
            if not cax:
                raise ValueError(f"{path}: cannot tell the channel axis of shape {a.shape}")
            if channel is None:
                if a.shape[cax[0]] != 1:
                    raise ValueError(f"{path} is a multi channel image but no color channel index was specified.")
                channel = 0
            if not 0 <= channel < a.shape[cax[0]]:
                raise ValueError(f"Color channel {channel} is out of range for {path} with color channels: 0 - {a.shape[cax[0]] - 1}")
            a = np.take(a, channel, axis=cax[0])
    else:
        a, _ = helper.load_image(path, time, channel)
        if a.ndim == 3:
            raise ValueError(f"{path}: multi-page file (Z stack); project it first with compute_zproj.py")
    if a.ndim != 2:
        raise ValueError(f"{path}: expected a single-channel 2-D image, got shape {a.shape}")
    if a.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"{path}: expected uint8/uint16 pixels, got {a.dtype}")
    return a        # uint8 images are widened at the ABI and flagged (input_bits=8): cv2.resize saturates to the source depth


def n_planes(path: str) -> int:
    """helper.get_image_dims(path).Z of the reference for the formats read here: pages of a TIFF, leading axis of a 3-D .npy"""
    if path.endswith(".npy"):
        a = np.load(path, mmap_mode="r")
        return a.shape[0] if a.ndim == 3 and a.shape[0] > 4 and a.shape[-1] > 4 else 1
    from PIL import Image
    from tmat_amd import helper
    try:
        with Image.open(path) as im:
            n = getattr(im, "n_frames", 1)
            desc = dict(getattr(im, "tag_v2", {}) or {}).get(270, "")
    except OSError:
        return 1
    if isinstance(desc, (tuple, list)):
        desc = desc[0] if desc else ""
    if isinstance(desc, bytes):
        desc = desc.decode("utf8", "replace")
    return helper.page_layout(desc, n)[1]            # SizeZ: pages of a time series or of channels are not Z slices


def find_inputs(in_root: Path):
    """compute_branches.py:547-566 -> (paths, is_stack): {stack id: [slice files] | multi-page file} or {stem: 2-D image file}"""
    from tmat_amd import zstacks as zs
    entries = sorted(glob(str(in_root / "*")))
    test_path = entries[0]
    if os.path.isdir(test_path) or n_planes(test_path) == 1:
        try:
            img_paths = zs.find_zstack_image_sequences(str(in_root))
            if any(len(seq) == 1 for seq in img_paths.values()):
                img_paths = {}          # not z stacks. probably projections.
        except zs.ZStackInputException:
            img_paths = {}
    else:
        try:
            img_paths = zs.find_zstack_files(str(in_root))
        except zs.ZStackInputException as exc:
            print(f"{FAIL} {exc}", flush=True)
            sys.exit(1)
    if img_paths:
        return img_paths, True
    return {Path(fp).stem: fp for fp in entries if os.path.isfile(fp) and n_planes(fp) == 1}, False


def load_stack(files, channel=None, time=None) -> np.ndarray:
    """(Z, H, W) uint8 / uint16 stack of one Z-stack entry (reference helper.load_image with a list of slice files or one
    multi-page file)"""
    from tmat_amd import helper
    if isinstance(files, str) and files.endswith(".npy"):
        a = np.load(files)
    else:
        a, _ = helper.load_image(files, time, channel)
    if a.ndim != 3:
        raise ValueError(f"{np.atleast_1d(files)[0]}: expected a Z stack, got shape {a.shape}")
    if a.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"{np.atleast_1d(files)[0]}: expected uint8/uint16 pixels, got {a.dtype}")
    if a.shape[0] < 2:
        raise ValueError(f"{np.atleast_1d(files)[0]}: a Z stack needs at least 2 slices")
    return a


def plan_image_2d(path: str, channel=None, time=None):
    """load_image_2d without the decode (--tiff-decoder device): a helper.PlaneSource of the plane, with load_image_2d's checks; .npy
    arrays are loaded as before"""
    from tmat_amd import helper
    if path.endswith(".npy"):
        return load_image_2d(path, channel, time)
    src = helper.plan_planes(path, time, channel)
    if len(src.shape) == 3:
        raise ValueError(f"{path}: multi-page file (Z stack); project it first with compute_zproj.py")
    if src.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"{path}: expected uint8/uint16 pixels, got {src.dtype}")
    return src


def plan_stack(files, channel=None, time=None):
    """load_stack without the decode (--tiff-decoder device), with its checks"""
    from tmat_amd import helper
    if isinstance(files, str) and files.endswith(".npy"):
        return load_stack(files, channel, time)
    src = helper.plan_planes(files, time, channel)
    if len(src.shape) != 3:
        raise ValueError(f"{np.atleast_1d(files)[0]}: expected a Z stack, got shape {src.shape}")
    if src.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"{np.atleast_1d(files)[0]}: expected uint8/uint16 pixels, got {src.dtype}")
    if src.shape[0] < 2:
        raise ValueError(f"{np.atleast_1d(files)[0]}: a Z stack needs at least 2 slices")
    return src


def make_stack_fn(handle):
    """run_sharded's stack_fn for --tiff-decoder device: the group's files are decoded on the device into one resident block
    (helper.load_planes_dev), shaped like the batch np.stack would give; a group that holds .npy arrays is stacked on the host"""
    from tmat_amd import helper

    def stack_fn(items):
        if all(isinstance(it, helper.PlaneSource) for it in items):
            dev = helper.load_planes_dev(handle, items)
            dev.shape = (len(items),) + items[0].shape
            return dev
        arrays = []
        for it in items:
            if isinstance(it, helper.PlaneSource):
                with helper.load_planes_dev(handle, [it]) as dev:
                    it = dev.download().reshape(it.shape)
            arrays.append(it)
        return np.stack(arrays).astype(np.uint16)
    return stack_fn


def resident(batch) -> bool:
    """a batch decoded on the device and still there (helper.DevPlanes), not a host array"""
    from tmat_amd import helper
    return isinstance(batch, helper.DevPlanes)


def make_load_fn(loader, paths, args):
    """run_sharded's load_fn over loader (load_image_2d or load_stack): an unreadable entry prints the failure and raises InputError"""
    from tmat_amd import branches

    def load_fn(img_id):
        try:
            return loader(paths[img_id], args.channel, args.time)
        except (OSError, ValueError) as error:
            print(f"{FAIL}{error}", flush=True)
            raise branches.InputError(str(error))
    return load_fn


def make_width_fn(config, paths):
    """run_sharded's width_fn.  image_width_microns: the option / config key, else per image from the file's metadata (reference
    compute_branches.py:184-212: img.shape[-1] * PhysicalPixelSizes.X; of a slice sequence: its first file), else the reference's
    failure message"""
    from tmat_amd import branches, helper

    def width_fn(img_id, img):
        width_um = config.get("image_width_microns")
        if width_um is None:
            px = helper.physical_pixel_sizes(str(np.atleast_1d(paths[img_id])[0])).X
            if px is None:
                print(f"{FAIL} The --image-width-microns parameter was not specified, and the pixel to micron conversion "
                      f"factor was not found in the image metadata ({img_id}). Specify --image-width-microns and try again. "
                      "Exiting...", flush=True)
                raise branches.InputError(img_id)
            width_um = img.shape[-1] * px
        return width_um
    return width_fn


def write_results(args, config, ids, gathered, out_root: Path, rank: int):
    """the CSV per threshold configuration and config.json (compute_branches.py:459-500, 596-600), written by rank 0"""
    from tmat_amd import branches
    created = set()
    for _, suffix in branches.threshold_grid(config):
        rows = gathered[suffix]
        if rank != 0:
            continue
        output_file = out_root / f"branching_analysis{suffix}.csv"
        n = 1
        while output_file.is_file() and str(output_file) not in created:
            n += 1
            output_file = out_root / f"branching_analysis{suffix}-{n}.csv"
        create_output_csv(output_file)
        created.add(str(output_file))
        with open(output_file, "a", encoding="utf-16") as f:
            wr = csv.writer(f, lineterminator="\n")
            for gidx, cnt, tot_um, avg_um in rows:
                wr.writerow([ids[gidx], cnt, tot_um, avg_um])
        print(f"Results saved to {output_file}.", flush=True)
    if rank == 0:
        config["time"], config["channel"] = getattr(args, "time", None), getattr(args, "channel", None)
        with open(get_unique_output_filepath(out_root / "config.json"), "w", encoding="utf8") as f:
            json.dump({k: v for k, v in config.items() if v is not None}, f, indent=4)
        print(f"{OK} Analysis complete.", flush=True)


def finish_distributed(ws: int):
    if ws > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


def run_stacks(args, config, paths, out_root: Path, rank: int, ws: int, local_rank: int):
    """Z-stack entries: the Sato branch (compute_branches.py:224-306) on this rank's share of the stacks"""
    from tmat_amd import _lib, branches, distributed, sato
    handle = _lib.Handle(None, local_rank)          # this branch needs no segmentation model
    hessian = getattr(args, "sato_hessian", "gaussian_derivatives")
    vis = bool(getattr(args, "visualizations", False))
    detect_well = bool(getattr(args, "detect_well", False))
    well_seed = int(getattr(args, "well_seed", 0) or 0)
    tree_vis = bool(getattr(args, "tree_visualizations", False))
    vis_width = int(getattr(args, "vis_width", 2000) or 2000)
    encoder = handle.png_encode if getattr(args, "png_encoder", "pil") == "device" else None
    handle.png_set_mode(getattr(args, "png_compression", "fast"))
    grid = branches.threshold_grid(config)
    suffix_of = {(cfg["thresh1"], cfg["thresh2"]): sfx for cfg, sfx in grid}
    ids = sorted(paths)
    fields = {}
    # Batch path (tmat_analyze_stack_batch_dev): consecutive stacks of one shape and width are uploaded once and go through the device
    # stages together, the host graph stage of a pass runs beside the device stages of the next, the threshold grid is swept from fields
    # that stay in HBM; --detect-well makes its masks from the resident chunk (sato.stack_well_masks_batch) and --tree-visualizations
    # takes geometry and overlays out of the same call.  TMAT_STACK_BATCH=0 keeps every stack on the per-stack path; stacks of a unique
    # shape always take it.
    batch_on = os.environ.get("TMAT_STACK_BATCH", STACK_BATCH_DEFAULT) != "0"

    def save_well_mask(img_id, well):
        # compute_branches.py:239-241 well_mask.png, from the masks the analysis itself uses
        (out_root / "visualizations" / img_id).mkdir(parents=True, exist_ok=True)
        if encoder is not None:
            (out_root / "visualizations" / img_id / "well_mask.png").write_bytes(encoder((well * 255).astype(np.uint8))[0])
        else:
            from PIL import Image
            Image.fromarray((well * 255).astype(np.uint8)).save(out_root / "visualizations" / img_id / "well_mask.png")

    device_decode = getattr(args, "tiff_decoder", "pil") == "device"
    load_fn, width_fn = make_load_fn(plan_stack if device_decode else load_stack, paths, args), make_width_fn(config, paths)

    def analyze_batch_fn(batch, width_um, thresh, ids):
        # one upload and one pass over the whole chunk and the whole grid; run_sharded then asks configuration by configuration
        if fields.get("batch") is not batch:
            fields.clear()
            fields["batch"] = batch
            sw_px, min_px, max_px = branches.graph_px_params(config, DOWNSAMPLE_WIDTH, width_um)
            pairs = [(cfg["thresh1"], cfg["thresh2"]) for cfg, _ in grid]
            n, per = len(batch), int(np.prod(batch.shape[1:]))
            rows_all = [[] for _ in pairs]
            # --tiff-decoder device: the decoded block is the resident chunk (run_sharded frees it); else one upload
            with (contextlib.nullcontext(sato.DevStacks(handle, batch.ptr, batch.shape)) if resident(batch) else sato.upload_stacks(handle, batch)) as dev:
                pruning = None
                if detect_well:
                    well, pruning = sato.stack_well_masks_batch(handle, dev, sato.dsamp_shape(batch.shape, DOWNSAMPLE_WIDTH), well_seed)
                    if vis:
                        for i, img_id in enumerate(ids):
                            save_well_mask(img_id, well[i])
                # the overlays of one call stay under a gigabyte of host memory, as on the 2-D route
                vh, vw = _lib.tree_canvas_shape(batch.shape[2], batch.shape[3], vis_width)
                step = branches.grid_images_per_call(len(pairs), vh * vw * 3) if tree_vis else n
                for i0 in range(0, n, step):
                    k = min(step, n - i0)
                    part = (C.c_void_p(dev.ptr.value + i0 * per * 2), (k,) + batch.shape[1:])
                    res = sato.analyze_stack_batch(handle, part, pairs, sw_px, min_px, max_px, bool(config.get("remove_isolated_branches", False)),
                                                   DOWNSAMPLE_WIDTH, hessian, pruning_masks=None if pruning is None else pruning[i0:i0 + k],
                                                   return_pictures=vis, tree=tree_vis, vis_width=vis_width)
                    res = res if isinstance(res, tuple) else (res,)
                    for t in range(len(pairs)):
                        rows_all[t] += res[0][t]
                    if vis:
                        for i, img_id in enumerate(ids[i0:i0 + k]):
                            vis_dir = out_root / "visualizations" / img_id
                            branches._save_png_unique(res[1][0][i], vis_dir, "original_image.png", encoder)
                            branches._save_png_unique(res[1][1][i], vis_dir, "vesselness_image.png", encoder)
                    if tree_vis:
                        # compute_branches.py:431-450: the files of every configuration, written while this call's overlays are held
                        for t, pair in enumerate(pairs):
                            for i, img_id in enumerate(ids[i0:i0 + k]):
                                bars = res[-1]["bars"][t][i]
                                if len(bars) == 0:
                                    print(f"No branches found for {img_id}.", flush=True)
                                branches.save_tree_pictures(res[-1]["overlays"][t][i], bars, out_root / "visualizations" / img_id, suffix_of[pair],
                                                            vis_width, encoder)
            fields["rows"] = {pair: rows_all[t] for t, pair in enumerate(pairs)}
        return [(i,) + tuple(r) for i, r in enumerate(fields["rows"][thresh])]

    def analyze_fn(batch, width_um, thresh, input_bits, ids):
        if batch_on and len(batch) > 1:
            return analyze_batch_fn(batch, width_um, thresh, ids)
        if resident(batch):         # the per-stack path works on host arrays: the decoded block is downloaded once
            batch = batch.host()
        # the vesselness image does not depend on the graph thresholds: one field per stack, swept over the grid
        sw_px, min_px, max_px = branches.graph_px_params(config, DOWNSAMPLE_WIDTH, width_um)
        rows = []
        if fields.get("batch") is not batch:            # run_sharded hands the same array to every configuration of the grid
            fields.clear()
            fields["batch"] = batch
        for i, st in enumerate(batch):
            if i not in fields:
                field = sato.stack_field(handle, st, DOWNSAMPLE_WIDTH, hessian)
                # --detect-well (compute_branches.py:231-243): the well mask of the resized max projection only prunes the graph here
                pruning = None
                if detect_well:
                    well, pruning = sato.stack_well_masks(handle, st, field.shape, well_seed)
                    if vis:
                        save_well_mask(ids[i], well)
                fields[i] = (field, pruning)
                if vis:
                    # compute_branches.py:228-229 original_image.png = the max projection, :303 vesselness_image.png: save_vis of the field
                    # this call has just computed, on the device
                    vis_dir = out_root / "visualizations" / ids[i]
                    branches._save_png_unique(handle.stage_pictures(st.max(0)), vis_dir, "original_image.png", encoder)
                    branches._save_png_unique(handle.stage_pictures(field), vis_dir, "vesselness_image.png", encoder)
            rows.append((i,) + sato.field_stats(handle, fields[i][0], thresh[0], thresh[1], sw_px, min_px, max_px,
                                                bool(config.get("remove_isolated_branches", False)), pruning_mask=fields[i][1]))
            if tree_vis:
                # compute_branches.py:431-450: the tree of the 0..255 field over the full-resolution max projection, scaled by W / 384 (:437)
                background = st.max(0)
                tree, bars, _ = branches.field_tree(handle, _lib.host_rescale255_f32(fields[i][0]), config, width_um, thresh, fields[i][1],
                                                    background.shape[1] / fields[i][0].shape[1])
                if len(bars) == 0:
                    print(f"No branches found for {ids[i]}.", flush=True)
                branches.save_tree_visualizations(handle, background, tree, bars, out_root / "visualizations" / ids[i], suffix_of[thresh], vis_width,
                                                  encoder)
        return rows

    def stack_chunk_ends(held_keys, key, st):
        # sato.chunk_stacks' rule on the stream of loaded stacks: one key per chunk, at most 8 stacks, the pass's device bytes plus the
        # resident chunk under the budget
        return sato.stack_chunk_ends(held_keys, key, st.shape, DOWNSAMPLE_WIDTH)

    # per-stack path: one stack per analysis call (chunk=1): a stack is the unit the reference streams, and it can be gigabytes
    try:
        gathered = branches.run_sharded(ids, load_fn, width_fn, analyze_fn, config, rank, ws, chunk=sato.STACK_PASS_MAX if batch_on else 1,
                                        log=lambda m: print(m, flush=True), pass_ids=True, chunk_ends=stack_chunk_ends if batch_on else None,
                                        stack_fn=make_stack_fn(handle) if device_decode else None)
    except distributed.RankFailed:
        handle.close()
        finish_distributed(ws)
        sys.exit(1)
    write_results(args, config, ids, gathered, out_root, rank)
    handle.close()
    finish_distributed(ws)


def main(args=None):
    if args is None:
        args = parse_branching_args({"default_config_path": DEFAULT_CONFIG_PATH})
        if not Path(args.config).is_file():
            print(f"{FAIL} Config file {args.config} does not exist.", flush=True)
            sys.exit(1)
        with open(args.config, "r", encoding="utf8") as fp:
            config = json.load(fp)
    else:
        config = {}
    ad = vars(args)
    if ad.get("png_compression", "fast") != "fast" and ad.get("png_encoder", "pil") != "device":
        print(f"{FAIL} --png-compression {ad['png_compression']} needs --png-encoder device.", flush=True)
        sys.exit(1)
    for prm in ("image_width_microns", "graph_thresh_1", "graph_thresh_2", "graph_smoothing_window", "min_branch_length",
                "max_branch_length", "remove_isolated_branches"):
        if prm not in config or ad.get(prm) is not None:
            config[prm] = ad.get(prm)
    model_cfg_path = config.get("model_cfg_path")
    if not model_cfg_path:
        cfgs = sorted(glob(str(PKG / "model_training" / "binary_segmentation" / "configs" / "unet_patch_segmentor_*.json")),
                      key=lambda s: int(Path(s).stem.rsplit("_", 1)[1]))
        model_cfg_path = cfgs[-1] if cfgs else ""
    if not Path(model_cfg_path).is_file():
        print(f"{FAIL}Model config file {model_cfg_path} does not exist.", flush=True)
        sys.exit(1)
    in_root, out_root = Path(args.in_root), Path(args.out_root)
    if not in_root.is_dir():
        print(f"{FAIL} Input directory {in_root} does not exist.", flush=True)
        sys.exit(1)
    try:
        out_root.mkdir(parents=True, exist_ok=True)
    except PermissionError as e:
        print(f"{FAIL} {e}", flush=True)
        sys.exit(1)
    if not glob(str(in_root / "*")):
        print(f"{FAIL}No images found in {in_root}", flush=True)
        sys.exit(1)
    paths, is_stack = find_inputs(in_root)
    if not paths:
        print(f"{FAIL}No images found in {in_root}", flush=True)
        sys.exit(1)
    # image_width_microns: the option / config key, else per image from the file's metadata (reference
    # compute_branches.py:184-212: img.shape[-1] * PhysicalPixelSizes.X), else the reference's failure message
    from tmat_amd import branches, distributed, models
    ws = distributed.world()[0]
    # host stages (thinning, DMT, MorseGraph) run on worker threads of every rank: share the cores between the ranks
    os.environ.setdefault("TMAT_HOST_THREADS", str(distributed.host_threads_per_rank(ws)))
    ws, rank, local_rank = distributed.init_process_group_from_env()
    if is_stack:
        run_stacks(args, config, paths, out_root, rank, ws, local_rank)
        return
    model = models.get_unet_patch_segmentor_from_cfg(model_cfg_path, device_id=local_rank)
    # models.py:636-637 normalises the image in predict(): the batched device path does it in front of the smooth prediction
    model.handle.set_input_norm(model.norm_mean, model.norm_std)
    detect_well = bool(getattr(args, "detect_well", False))
    well_seed = int(getattr(args, "well_seed", 0) or 0)
    # --png-encoder device: every PNG below goes through the handle's encoder, batched by shape; pil (the default): Pillow, file by file
    encoder = model.handle.png_encode if getattr(args, "png_encoder", "pil") == "device" else None
    model.handle.png_set_mode(getattr(args, "png_compression", "fast"))

    # ids are file stems, as in the reference (compute_branches.py:565-569: two files with one stem are one entry there too)
    ids = sorted(paths)
    device_decode = getattr(args, "tiff_decoder", "pil") == "device"
    load_fn, width_fn = make_load_fn(plan_image_2d if device_decode else load_image_2d, paths, args), make_width_fn(config, paths)

    well_cache = {}

    # --tree-visualizations (compute_branches.py:431-450): the pictures are written per image and threshold configuration inside analyze_fn
    tree_vis = bool(getattr(args, "tree_visualizations", False))
    vis_width = int(getattr(args, "vis_width", 2000) or 2000)
    suffix_of = {(cfg["thresh1"], cfg["thresh2"]): sfx for cfg, sfx in branches.threshold_grid(config)}

    # --visualizations (compute_branches.py:315, 331, 347, 348, 364): the pictures do not depend on the graph thresholds -- they come out
    # of the batched call of the first configuration a batch sees (run_sharded hands the same array to every configuration of the grid)
    vis = bool(getattr(args, "visualizations", False))
    vis_cache = {}

    def want_pictures(batch):
        if not vis or vis_cache.get("batch") is batch:
            return False
        vis_cache["batch"] = batch
        return True

    def write_pictures(ids, pictures, well=None):
        if encoder is not None:         # the whole batch's pictures in one encoder call
            items = []
            for i, img_id in enumerate(ids):
                items += branches.stage_picture_items(pictures[i], out_root / "visualizations" / img_id, None if well is None else well[i])
            branches.write_png_batch(items, encoder)
            return
        for i, img_id in enumerate(ids):
            branches.save_stage_pictures(pictures[i], out_root / "visualizations" / img_id, None if well is None else well[i])

    # The threshold grid from ONE pass of the network (branches.analyze_batch_grid): the first configuration run_sharded asks of a batch
    # makes the grid call -- rows of every pair, the pictures written then and there --, the others are served from its rows (run_sharded
    # hands the same array to every configuration of the grid).  The pictures go through in sub-batches that keep the picture buffers
    # of one call under branches.grid_images_per_call's budget; only rows are held for the batch.
    pairs = branches.grid_pairs(config)
    grid_cache = {}
    warn_fn = lambda m: print(f"\033[93m[WARNING]\033[0m {m}", flush=True)       # noqa: E731

    def grid_rows(batch, width_um, input_bits, ids):
        if detect_well:
            # --detect-well through the batch pipeline (branches.analyze_batch_well): masks and pictures do not depend on the thresholds
            rows_by, well, _, *pictures = branches.analyze_batch_well(model.handle, batch, config, width_um, model.ds_ratio, input_bits=input_bits,
                                                                      well_seed=well_seed, warn=warn_fn, stage_pictures=vis, pairs=pairs)
            if vis:
                write_pictures(ids, pictures[0], well)
            return rows_by
        on_device = tree_vis and encoder is not None        # --png-encoder device: the files come out of the call, nothing is uploaded again
        per = branches.grid_picture_bytes(batch.shape[1:], model.ds_ratio, vis_width, not on_device, on_device, on_device) if tree_vis else 0
        step = branches.grid_images_per_call(len(pairs), per) if per else len(batch)
        rows_by = {p: [] for p in pairs}
        for i0 in range(0, len(batch), step):
            sub_ids = ids[i0:i0 + step]
            sub = batch.part(i0, min(step, len(batch) - i0)) if resident(batch) else batch[i0:i0 + step]      # resident: tmat_analyze_batch_grid_dev
            rb, ex = branches.analyze_batch_grid(model.handle, sub, config, width_um, model.ds_ratio, pairs, first_index=i0,
                                                 input_bits=input_bits, tree=tree_vis, vis_width=vis_width, stage_pictures=vis,
                                                 tree_png=on_device, barcode_png=on_device, raw_overlays=not on_device, budget=1 << 62)
            if vis:
                write_pictures(sub_ids, ex["pictures"])
            for p in pairs:
                rows_by[p] += rb[p]
                if not tree_vis:
                    continue
                items = []
                for i, img_id in enumerate(sub_ids):
                    br, vis_dir = ex["bars"][p][i], out_root / "visualizations" / img_id
                    if len(br) == 0:            # the reference prints this and skips its plots (compute_branches.py:426-429)
                        print(f"No branches found for {img_id}.", flush=True)
                    elif on_device:
                        items += [(ex["tree_png"][p][i], vis_dir, f"morse_tree{suffix_of[p]}.png"),
                                  (ex["barcode_png"][p][i], vis_dir, f"barcode{suffix_of[p]}.png")]
                    else:
                        branches.save_tree_pictures(ex["overlays"][p][i], br, vis_dir, suffix_of[p], vis_width)
                if items:
                    branches.write_png_batch(items, encoder)
        return rows_by

    def analyze_fn(batch, width_um, thresh, input_bits, ids):
        if resident(batch) and detect_well:         # the -w routes take host arrays: the decoded block is downloaded once
            batch = batch.host()
        if not (detect_well and tree_vis):
            if grid_cache.get("batch") is not batch:
                grid_cache.clear()
                grid_cache["batch"] = batch
                grid_cache["rows"] = grid_rows(batch, width_um, input_bits, ids)
            return grid_cache["rows"][thresh]
        pics = want_pictures(batch)
        # with --tree-visualizations the pictures need the fields themselves: the staged entry points, image by image
        # --detect-well (compute_branches.py:318-337): the fields do not depend on the graph thresholds -- one staged pass per
        # batch (run_sharded hands the same array to every configuration of the grid), then the graph stages per configuration
        if well_cache.get("batch") is not batch:
            well_cache.clear()
            well_cache["batch"] = batch
            well_cache["fields"], well_cache["backgrounds"] = branches.well_fields(
                model.handle, batch, model.ds_ratio, input_bits, well_seed, warn=warn_fn, return_backgrounds=True)
        if pics:
            # this route stays staged (its overlays are drawn over the f32 background): the pictures come from one batched call with its masks
            wells = np.stack([f[2] for f in well_cache["fields"]])
            _, ex = branches.analyze_batch_ex(model.handle, batch, config, width_um, model.ds_ratio, thresh=thresh, input_bits=input_bits,
                                              well_masks=wells, pruning_masks=np.stack([f[1] for f in well_cache["fields"]]), stage_pictures=True)
            write_pictures(ids, ex["pictures"], wells)
        # the tree of each pruned graph over the image's own down-sampled picture; count, total and average come out of the same
        # call (tmat_morse_tree shares tmat_morse_stats' code), so the rows are well_rows' rows
        rows = []
        for i, ((f255, pruning, _), background) in enumerate(zip(well_cache["fields"], well_cache["backgrounds"])):
            tree, bars, stats = branches.field_tree(model.handle, f255, config, width_um, thresh, pruning, background.shape[1] / f255.shape[1])
            if len(bars) == 0:
                print(f"No branches found for {ids[i]}.", flush=True)
            branches.save_tree_visualizations(model.handle, background, tree, bars, out_root / "visualizations" / ids[i], suffix_of[thresh], vis_width,
                                              encoder)
            rows.append((i,) + stats)
        return rows

    try:
        gathered = branches.run_sharded(ids, load_fn, width_fn, analyze_fn, config, rank, ws,
                                        log=lambda m: print(m, flush=True), pass_ids=True,
                                        stack_fn=make_stack_fn(model.handle) if device_decode else None)
    except distributed.RankFailed:          # the failing rank has printed the reference's message; every rank exits with code 1
        model.handle.close()
        finish_distributed(ws)
        sys.exit(1)
    write_results(args, config, ids, gathered, out_root, rank)
    model.handle.close()
    finish_distributed(ws)


if __name__ == "__main__":
    main()
