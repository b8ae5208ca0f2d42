#!/usr/bin/env python3
"""Throughput of the --detect-well form of the 2-D branch: the staged path (branches.well_fields + well_rows, image by image through
the staged entry points, the superellipse search in numpy) against branches.analyze_batch_well (the masks of the whole batch fitted on
the device, then the two-stage batch pipeline with the masks).  Prints one JSON line; --out FILE also writes it there.

--n synthetic 1024 x 1024 projections inside a bright well -- round wells (the fit picks n = 2) and rounded-square wells (n = 8)
alternate; 16 distinct images, repeated.  One warm-up call of each path on 8 images, then --repeats timed calls each, alternating; wall
clock around the synchronous calls.  `mask_share` is the part of analyze_batch_well spent in tmat_preprocess_batch +
make_well_masks_batch (timed in a call of their own; the pipeline is then run with those masks).  The rows of both paths are compared.

    python tools/bench_well.py [--n 64] [--repeats 3] [--seed 7] [--out profiles/well_batch_bench.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
for p in (REPO, REPO / "tissue-model-analysis-tools_amd", REPO / "tools"):
    sys.path.insert(0, str(p))

CFG = dict(graph_thresh_1=5, graph_thresh_2=10, graph_smoothing_window=12, min_branch_length=12, remove_isolated_branches=False)


def well_image(index: int, size: int = 1024) -> np.ndarray:
    """a synthetic projection whose vessels sit inside a bright well: round for even indices, a rounded square for odd ones"""
    from tmat_amd import synth
    img = synth.synth_image(index, size).astype(np.float64)
    yy, xx = np.mgrid[0:size, 0:size]
    u, v = (xx - size * 0.51) / (size * 0.45), (yy - size * 0.49) / (size * 0.45)
    inside = (u ** 2 + v ** 2 < 1) if index % 2 == 0 else (u ** 8 + v ** 8 < 1)
    return np.clip(np.where(inside, img + 12000.0, 0.0), 0, 65535).astype(np.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from tmat_amd import _lib, branches, synth

    distinct = [well_image(i) for i in range(min(16, args.n))]
    imgs = np.stack([distinct[i % len(distinct)] for i in range(args.n)])
    handle = _lib.Handle(synth.pack_weights(synth.synth_weights(0)), 0, 0)
    quiet = lambda m: None      # noqa: E731

    def staged(batch):
        fields = branches.well_fields(handle, batch, 0.625, 16, args.seed, warn=quiet)
        return branches.well_rows(handle, fields, CFG, 500.0), fields

    def masks_of(batch):
        n, H, W = batch.shape
        x = np.empty((n, int(round(W * 0.625)), int(round(H * 0.625))), np.float32)
        _lib.check(_lib.lib().tmat_preprocess_batch(handle.raw, _lib.ptr(batch), n, H, W, 0.625, _lib.ptr(x)), "tmat_preprocess_batch")
        from tmat_amd import well_mask_generation as wmg
        well, shrunken = wmg.make_well_masks_batch(x, handle, seed=args.seed, warn=quiet)
        fshape = branches.dsamp_shape((H, W))
        return well, np.stack([wmg._resize_nearest(~shrunken[i], fshape) for i in range(n)])

    try:
        staged(imgs[:8])
        branches.analyze_batch_well(handle, imgs[:8], CFG, 500.0, well_seed=args.seed, warn=quiet)
        t_staged, t_batched, t_masks = [], [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            rows_s, fields = staged(imgs)
            t_staged.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            masks = masks_of(imgs)
            t1 = time.perf_counter()
            rows_b, _, _ = branches.analyze_batch_well(handle, imgs, CFG, 500.0, well_seed=args.seed, warn=quiet, masks=masks)
            t2 = time.perf_counter()
            t_masks.append(t1 - t0)
            t_batched.append(t2 - t0)
        same = rows_b == rows_s and all(np.array_equal(masks[0][i], fields[i][2]) and np.array_equal(masks[1][i], fields[i][1]) for i in range(args.n))
        used = sum(not masks[0][i].all() for i in range(args.n))
    finally:
        handle.close()
    ms, mb, mm = float(np.median(t_staged)), float(np.median(t_batched)), float(np.median(t_masks))
    res = dict(metric="well_images_per_s", n_images=args.n, image=[1024, 1024], repeats=args.repeats, well_seed=args.seed,
               staged_images_per_s=args.n / ms, batched_images_per_s=args.n / mb, speedup=ms / mb, mask_share=mm / mb,
               staged_s=[round(t, 4) for t in t_staged], batched_s=[round(t, 4) for t in t_batched], masks_s=[round(t, 4) for t in t_masks],
               rows_and_masks_equal=bool(same), images_with_a_well_mask=int(used), branches_total=int(sum(r[1] for r in rows_b)))
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).write_text(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
