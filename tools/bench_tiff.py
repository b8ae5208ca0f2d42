#!/usr/bin/env python3
"""What decoding TIFF input on the device buys.  Needs a GPU.  Prints one JSON line and, without --quick, writes
profiles/tiff_bench.json.

* workloads: --n images of 1024 x 1024 uint16 (synth.synth_image) as single-page files, and --stacks stacks of 16 x 2048 x 2048 as
  multi-page files (each plane four synthetic images side by side with a per-plane offset), each written by Pillow as uncompressed, LZW
  and LZW + horizontal predictor.
* two routes up to "pixels resident in device memory as (n, H, W) uint16", from files on disk:
    parent  Pillow decode on one thread, np.stack(...).astype(np.uint16), one upload (tmat_dev_upload)       -- wall clock
    device  read the file bytes, tmat_tiff_decode_batch_dev_timed: upload and kernels as HIP-event intervals  -- wall clock and events
  The routes alternate; medians of --repeats after one warm-up each.  `spread` is the largest difference between two repeats of the
  same route; a difference counts when it exceeds five times it.  The device pixels are checked against the parent's.
* end to end: scripts/compute_zproj.py on the stacks and scripts/compute_branches.py on the images, LZW + predictor, --tiff-decoder pil
  against device, alternating, --rounds rounds, wall clock of the whole process.

    python tools/bench_tiff.py [--n 64] [--stacks 8] [--repeats 5] [--rounds 3] [--quick]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
for p in (REPO, REPO / "tissue-model-analysis-tools_amd", REPO / "tools"):
    sys.path.insert(0, str(p))

FORMATS = {"uncompressed": ("raw", False), "lzw": ("tiff_lzw", False), "lzw_predictor": ("tiff_lzw", True)}


def write_files(root, name, groups, fmt):
    """groups: a list of page lists -> the files' paths"""
    from PIL import Image
    comp, pred = FORMATS[fmt]
    d = Path(root) / name / fmt
    d.mkdir(parents=True)
    paths = []
    for i, pages in enumerate(groups):
        ims = [Image.fromarray(p) for p in pages]
        kw = dict(format="TIFF", compression=comp, tiffinfo={317: 2} if pred else {})
        if len(ims) > 1:
            kw.update(save_all=True, append_images=ims[1:])
        paths.append(d / f"{name}_{i:03d}.tif")
        ims[0].save(paths[-1], **kw)
    return paths


def parent_route(handle, paths, dev, shape):
    from PIL import Image
    from tmat_amd import _lib
    t0 = time.perf_counter()
    planes = []
    for p in paths:
        with Image.open(p) as im:
            for k in range(getattr(im, "n_frames", 1)):
                im.seek(k)
                planes.append(np.array(im))
    t1 = time.perf_counter()
    batch = np.stack(planes).astype(np.uint16)
    t2 = time.perf_counter()
    _lib.check(_lib.lib().tmat_dev_upload(handle.raw, dev, _lib.ptr(batch), batch.nbytes), "tmat_dev_upload")
    t3 = time.perf_counter()
    assert batch.shape == shape
    return dict(decode_ms=(t1 - t0) * 1e3, stack_ms=(t2 - t1) * 1e3, upload_ms=(t3 - t2) * 1e3, total_ms=(t3 - t0) * 1e3), batch


def device_route(handle, paths, pages, dev, shape):
    t0 = time.perf_counter()
    files = [Path(p).read_bytes() for p in paths]
    t1 = time.perf_counter()
    planes = [(i, k) for i in range(len(files)) for k in range(pages)]
    bits, status, ms = handle.tiff_decode_dev_timed(files, planes, shape[1], shape[2], dev)
    t2 = time.perf_counter()
    assert bits == 16 and not status.any(), status
    return dict(read_ms=(t1 - t0) * 1e3, call_ms=(t2 - t1) * 1e3, upload_event_ms=ms["upload"], kernels_event_ms=ms["kernels"],
                total_ms=(t2 - t0) * 1e3, file_bytes=sum(map(len, files)))


def spread(values):
    return float(max(values) - min(values)) if len(values) > 1 else 0.0


def compare(handle, paths, pages, shape, repeats):
    from tmat_amd import _lib
    L = _lib.lib()
    nbytes = int(np.prod(shape)) * 2
    dev = C.c_void_p()
    _lib.check(L.tmat_dev_alloc(handle.raw, nbytes, C.byref(dev)), "tmat_dev_alloc")
    try:
        _, want = parent_route(handle, paths, dev, shape)                  # warm-up, and the reference pixels
        device_route(handle, paths, pages, dev, shape)
        got = np.empty(shape, np.uint16)
        _lib.check(L.tmat_dev_download(handle.raw, _lib.ptr(got), dev, nbytes), "tmat_dev_download")
        same = bool(np.array_equal(got, want))
        par, devr = [], []
        for _ in range(repeats):
            par.append(parent_route(handle, paths, dev, shape)[0])
            devr.append(device_route(handle, paths, pages, dev, shape))
    finally:
        L.tmat_dev_free(handle.raw, dev)
    med = lambda rows, k: float(np.median([r[k] for r in rows]))       # noqa: E731
    p_tot, d_tot = [r["total_ms"] for r in par], [r["total_ms"] for r in devr]
    sp = max(spread(p_tot), spread(d_tot))
    diff = float(np.median(p_tot) - np.median(d_tot))
    kern = med(devr, "kernels_event_ms")
    return dict(planes=shape[0], shape=list(shape[1:]), pixels_equal_the_parent_route=same,
                parent_ms={k: med(par, k) for k in par[0]}, device_ms={k: med(devr, k) for k in devr[0] if k != "file_bytes"},
                bytes_uploaded_over_raw=devr[0]["file_bytes"] / nbytes, decoded_GB_per_s_kernels=nbytes / kern / 1e6 if kern > 0 else None,
                decoded_GB_per_s_device_route=nbytes / float(np.median(d_tot)) / 1e6, decoded_GB_per_s_parent_route=nbytes / float(np.median(p_tot)) / 1e6,
                spread_ms=sp, parent_minus_device_ms=diff, difference_counts=bool(abs(diff) > 5 * sp),
                verdict="device faster" if diff > 5 * sp else "parent faster" if -diff > 5 * sp else "tie")


def script_rounds(script, args, rounds):
    env = dict(os.environ, TMAT_SYNTHETIC_WEIGHTS="1")
    times = {"pil": [], "device": []}
    with tempfile.TemporaryDirectory() as out:
        for r in range(rounds + 1):                                         # round 0 warms the file cache and the code objects
            for dec in ("pil", "device"):
                t0 = time.perf_counter()
                res = subprocess.run([sys.executable, str(REPO / "tissue-model-analysis-tools_amd" / "scripts" / script)] +
                                     [a.replace("OUT", f"{out}/{dec}_{r}") for a in args] + ["--tiff-decoder", dec],
                                     capture_output=True, text=True, env=env, timeout=1200)
                if res.returncode != 0:
                    raise RuntimeError(res.stdout[-2000:] + res.stderr[-2000:])
                if r:
                    times[dec].append(time.perf_counter() - t0)
    sp = max(spread(times["pil"]), spread(times["device"]))
    diff = float(np.median(times["pil"]) - np.median(times["device"]))
    return dict(pil_s=float(np.median(times["pil"])), device_s=float(np.median(times["device"])), spread_s=sp, pil_minus_device_s=diff,
                difference_counts=bool(abs(diff) > 5 * sp), rounds=rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--stacks", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="8 images, 1 stack of 4 x 512 x 512, 2 repeats, 1 round, no file written")
    a = ap.parse_args()
    Z, side = 16, 2048
    if a.quick:
        a.n, a.stacks, a.repeats, a.rounds, Z, side = 8, 1, 2, 1, 4, 512
    from tmat_amd import _lib, synth
    distinct = [synth.synth_image(i, 1024).astype(np.uint16) for i in range(min(16, a.n))]
    images = [[distinct[i % len(distinct)]] for i in range(a.n)]
    tile = side // 1024 if side >= 1024 else 1
    base = [np.tile(d, (tile, tile))[:side, :side] for d in distinct[:4]]
    stacks = [[(base[(s + z) % len(base)] + np.uint16(17 * z + s)).astype(np.uint16) for z in range(Z)] for s in range(a.stacks)]
    res = dict(images=a.n, stacks=a.stacks, stack_shape=[Z, side, side], repeats=a.repeats)
    handle = _lib.Handle(None, 0)
    ok = True
    try:
        with tempfile.TemporaryDirectory() as root:
            res["workloads"] = {}
            paths = {}
            for fmt in FORMATS:
                paths["images", fmt] = write_files(root, "images", images, fmt)
                paths["stacks", fmt] = write_files(root, "stacks", stacks, fmt)
                res["workloads"][fmt] = dict(images=compare(handle, paths["images", fmt], 1, (a.n, 1024, 1024), a.repeats),
                                             stacks=compare(handle, paths["stacks", fmt], Z, (a.stacks * Z, side, side), a.repeats))
                ok = ok and all(w["pixels_equal_the_parent_route"] for w in res["workloads"][fmt].values())
            handle.close()
            handle = None
            res["end_to_end"] = dict(
                compute_zproj=script_rounds("compute_zproj.py", [str(paths["stacks", "lzw_predictor"][0].parent), "OUT", "-m", "max"], a.rounds),
                compute_branches=script_rounds("compute_branches.py", [str(paths["images", "lzw_predictor"][0].parent), "OUT",
                                                                       "--image-width-microns", "500"], a.rounds))
    finally:
        if handle is not None:
            handle.close()
    res["ok"] = ok
    print(json.dumps(res))
    if not a.quick:
        (REPO / "profiles" / "tiff_bench.json").write_text(json.dumps(res, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
