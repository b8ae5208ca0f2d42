#!/usr/bin/env python3
"""What the stage pictures of --visualizations cost: three forms of one workload in one process, alternated round by round.

    (a) branches.analyze_batch                                        the rows alone
    (b) branches.analyze_batch_ex(stage_pictures=True)                the rows and the (n, 4, h, w) pictures out of the same passes
    (c) analyze_batch, then branches.stage_pictures_staged per image  the way --visualizations worked before: a second network pass per image

--n synthetic 1024 x 1024 projections (synth.synth_image; 16 distinct images, repeated).  One warm-up call of each form on 8 images, then
--rounds rounds of (a), (b), (c) in this order; wall clock around the synchronous calls, every round printed to stderr and kept in the
result so that the spread is visible.  PNG encoding is timed on its own (branches.save_stage_pictures of form (b)'s pictures into a
temporary directory) and is part of none of the three.  The rows of (a) and (b) must be equal: exit code 1 if they are not.  Needs a
GPU.  Prints one JSON line; --out FILE also writes it there.

    python tools/bench_vis.py [--n 64] [--rounds 3] [--out profiles/vis_bench.json]
"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
for p in (REPO, REPO / "tissue-model-analysis-tools_amd", REPO / "tools"):
    sys.path.insert(0, str(p))

CFG = dict(graph_thresh_1=5, graph_thresh_2=10, graph_smoothing_window=12, min_branch_length=12, remove_isolated_branches=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3")
    from tmat_amd import _lib, branches, synth

    distinct = [synth.synth_image(i, 1024) for i in range(min(16, args.n))]
    imgs = np.stack([distinct[i % len(distinct)] for i in range(args.n)])
    handle = _lib.Handle(synth.pack_weights(synth.synth_weights(0)), 0, 0)      # no GPU: TmatError here

    def form_a(batch):
        return branches.analyze_batch(handle, batch, CFG, 500.0), None

    def form_b(batch):
        rows, ex = branches.analyze_batch_ex(handle, batch, CFG, 500.0, stage_pictures=True)
        return rows, ex["pictures"]

    def form_c(batch):
        rows = branches.analyze_batch(handle, batch, CFG, 500.0)
        return rows, [branches.stage_pictures_staged(handle, im) for im in batch]

    forms = (("a", form_a), ("b", form_b), ("c", form_c))
    times = {k: [] for k, _ in forms}
    out = {}
    try:
        for _, f in forms:
            f(imgs[:8])
        for r in range(args.rounds):
            for k, f in forms:
                t0 = time.perf_counter()
                out[k] = f(imgs)
                times[k].append(time.perf_counter() - t0)
            print(f"[bench_vis] round {r + 1}/{args.rounds}: " + ", ".join(f"({k}) {times[k][-1]:.3f} s = {args.n / times[k][-1]:.2f} images/s"
                                                                           for k, _ in forms), file=sys.stderr, flush=True)
        with tempfile.TemporaryDirectory() as d:
            t0 = time.perf_counter()
            for i in range(args.n):
                branches.save_stage_pictures(out["b"][1][i], Path(d) / f"img_{i}")
            t_png = time.perf_counter() - t0
    finally:
        handle.close()
    same_rows = out["a"][0] == out["b"][0]
    same_pics = all(np.array_equal(out["b"][1][i], np.stack(out["c"][1][i])) for i in range(args.n))
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = dict(metric="vis_images_per_s", n_images=args.n, image=[1024, 1024], rounds=args.rounds,
               a_analyze_batch_images_per_s=args.n / med["a"], b_with_stage_pictures_images_per_s=args.n / med["b"],
               c_staged_per_image_images_per_s=args.n / med["c"], b_over_a=med["b"] / med["a"], c_over_a=med["c"] / med["a"],
               a_s=[round(t, 4) for t in times["a"]], b_s=[round(t, 4) for t in times["b"]], c_s=[round(t, 4) for t in times["c"]],
               png_encode_s=round(t_png, 4), png_encode_ms_per_image=round(1e3 * t_png / args.n, 3),
               rows_equal=bool(same_rows), pictures_b_equal_c=bool(same_pics), branches_total=int(sum(r[1] for r in out["a"][0])))
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).write_text(line + "\n")
    return 0 if same_rows else 1


if __name__ == "__main__":
    sys.exit(main())
