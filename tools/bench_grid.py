#!/usr/bin/env python3
"""What sweeping the threshold grid from one pass of the network buys.  Needs a GPU.  Prints one JSON line and, without
--quick, writes profiles/grid_bench.json.

* rows only, --n synthetic 1024 x 1024 images, G in {1, 4, 9, 25} pairs (square grids over graph_thresh_1 x graph_thresh_2): the per-pair
  loop of analyze_batch -- one full pass of the network per pair, what every caller did before -- against ONE analyze_batch_grid call,
  alternating in one session, --rounds rounds each after a warm-up of both, wall clock.  Reported per G: the times, images/s (images of
  the batch per second: the grid's G results per image count once), the loop's round-to-round spread, and the two conditions -- at
  G = 1 the grid call's median lies inside the loop's range, at G = 9 it beats the loop by more than the loop's spread.
* with TMAT_TRACE=1 in the environment the library's per-pass trace lines of the grid calls are read back from stderr: the median
  "collect + Morse" milliseconds of a pass (the host graph stage over pairs x images) beside the milliseconds the coordinator waited
  for the GPU, per G.  If the host stage outlasts the GPU pass at G = 25 it shows here.
* trees at --vis-width for G = 4: the grid call with raw overlays, files made by PIL (morse_tree + barcode per image and pair), against
  the grid call with tree_png / barcode_png, file bytes written as they come -- the same rounds.
* --merge-bench FILE: bench.py result lines of one session, each prefixed "parent " or "branch " (tools/bench_overlay.py:bench_series).

    python tools/bench_grid.py [--n 32] [--rounds 3] [--vis-width 2000] [--quick]
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
for p in (REPO, REPO / "tissue-model-analysis-tools_amd", REPO / "tools"):
    sys.path.insert(0, str(p))

CFG = dict(graph_smoothing_window=12, min_branch_length=12, remove_isolated_branches=False)


def square_grid(G):
    side = int(round(G ** 0.5))
    assert side * side == G, G
    t1 = [5.0] if side == 1 else np.linspace(1.0, 9.0, side).tolist()
    t2 = [10.0] if side == 1 else np.linspace(4.0, 20.0, side).tolist()
    return [(a, b) for a in t1 for b in t2]


class StderrCapture:
    """the C library's trace lines (fprintf to stderr) of the calls made inside the block; inactive without TMAT_TRACE=1"""

    def __init__(self, active):
        self.active, self.text = active, ""

    def __enter__(self):
        if self.active:
            sys.stderr.flush()
            self.tmp = tempfile.TemporaryFile(mode="w+b")
            self.saved = os.dup(2)
            os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        if self.active:
            os.dup2(self.saved, 2)
            os.close(self.saved)
            self.tmp.seek(0)
            self.text = self.tmp.read().decode(errors="replace")
            self.tmp.close()
        return False


def trace_summary(text):
    host = [float(m) for m in re.findall(r"collect \+ Morse ([0-9.]+) ms", text)]
    gpu = [float(m) for m in re.findall(r"waited ([0-9.]+) ms for the GPU", text)]
    jobs = [float(m) for m in re.findall(r"GPU, ([0-9.]+) ms for host jobs", text)]
    if not host:
        return None
    return dict(passes=len(host), collect_morse_ms_per_pass_median=float(np.median(host)), collect_morse_ms_per_pass_max=max(host),
                waited_for_gpu_ms_per_pass_median=float(np.median(gpu)) if gpu else None,
                waited_for_host_jobs_ms_per_pass_median=float(np.median(jobs)) if jobs else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--vis-width", type=int, default=2000)
    ap.add_argument("--grids", type=int, nargs="+", default=[1, 4, 9, 25])
    ap.add_argument("--quick", action="store_true", help="8 images, G in {1, 4}, trees 600 wide, no file written")
    ap.add_argument("--merge-bench", type=str, default=None, metavar="FILE")
    a = ap.parse_args()
    if a.quick:
        a.n, a.grids, a.vis_width = 8, [1, 4], 600
    trace = os.environ.get("TMAT_TRACE", "0") not in ("", "0")
    from bench_overlay import bench_series
    from tmat_amd import _lib, branches, synth

    distinct = [synth.synth_image(i, 1024) for i in range(min(16, a.n))]
    imgs = np.stack([distinct[i % len(distinct)] for i in range(a.n)])
    handle = _lib.Handle(synth.pack_weights(synth.synth_weights(0)), 0, 0)
    res = dict(images=a.n, rounds=a.rounds, vis_width=a.vis_width, trace=trace, host_threads=os.environ.get("TMAT_HOST_THREADS"))
    ok = True
    try:
        res["grids"] = {}
        for G in a.grids:
            pairs = square_grid(G)

            def loop():
                return {p: branches.analyze_batch(handle, imgs, CFG, 500.0, thresh=p) for p in pairs}

            def grid():
                return branches.analyze_batch_grid(handle, imgs, CFG, 500.0, pairs=pairs)[0]

            same = loop() == grid()                                             # warm-up of both, and the rows agree
            t_loop, t_grid, traces = [], [], ""
            for r in range(a.rounds):
                t0 = time.perf_counter()
                loop()
                t_loop.append(time.perf_counter() - t0)
                with StderrCapture(trace) as cap:
                    t0 = time.perf_counter()
                    grid()
                    t_grid.append(time.perf_counter() - t0)
                traces += cap.text
                print(f"[bench_grid] G = {G} round {r + 1}/{a.rounds}: per-pair loop {t_loop[-1]:.3f} s, grid call {t_grid[-1]:.3f} s", file=sys.stderr, flush=True)
            ml, mg, spread = float(np.median(t_loop)), float(np.median(t_grid)), max(t_loop) - min(t_loop)
            e = dict(pairs=G, loop_s=t_loop, grid_s=t_grid, loop_images_per_s=a.n / ml, grid_images_per_s=a.n / mg, loop_round_to_round_spread_s=spread,
                     loop_minus_grid_median_s=ml - mg, speedup=ml / mg, rows_equal=bool(same),
                     grid_median_inside_loop_range=bool(min(t_loop) <= mg <= max(t_loop)),
                     grid_beats_loop_by_more_than_loop_spread=bool(ml - mg > spread))
            if trace:
                e["trace"] = trace_summary(traces)
            res["grids"][str(G)] = e
            ok = ok and same
        if "1" in res["grids"]:
            res["condition_a_g1_inside_spread"] = res["grids"]["1"]["grid_median_inside_loop_range"]
        if "9" in res["grids"]:
            res["condition_b_g9_beats_loop"] = res["grids"]["9"]["grid_beats_loop_by_more_than_loop_spread"]

        # ---- trees, G = 4 ----
        pairs = square_grid(4)

        def trees_pil(d):
            rows, ex = branches.analyze_batch_grid(handle, imgs, CFG, 500.0, pairs=pairs, tree=True, vis_width=a.vis_width)
            for t, p in enumerate(pairs):
                for i in range(a.n):
                    branches.save_tree_pictures(ex["overlays"][p][i], ex["bars"][p][i], Path(d) / f"img_{i}", f"_{t}", a.vis_width)
            return rows

        def trees_dev(d):
            rows, ex = branches.analyze_batch_grid(handle, imgs, CFG, 500.0, pairs=pairs, tree_png=True, barcode_png=True, raw_overlays=False,
                                                   vis_width=a.vis_width)
            for t, p in enumerate(pairs):
                for i in range(a.n):
                    if len(ex["bars"][p][i]):
                        vdir = Path(d) / f"img_{i}"
                        vdir.mkdir(parents=True, exist_ok=True)
                        (vdir / f"morse_tree_{t}.png").write_bytes(ex["tree_png"][p][i])
                        (vdir / f"barcode_{t}.png").write_bytes(ex["barcode_png"][p][i])
            return rows

        t_pil, t_dev = [], []
        with tempfile.TemporaryDirectory() as d:
            same = trees_pil(Path(d) / "warm_pil") == trees_dev(Path(d) / "warm_dev")
            n_files = len(list((Path(d) / "warm_dev").rglob("*.png")))
            same = same and n_files == len(list((Path(d) / "warm_pil").rglob("*.png")))
            for r in range(a.rounds):
                t0 = time.perf_counter()
                trees_pil(Path(d) / f"r{r}_pil")
                t_pil.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                trees_dev(Path(d) / f"r{r}_dev")
                t_dev.append(time.perf_counter() - t0)
                print(f"[bench_grid] trees round {r + 1}/{a.rounds}: raw + PIL {t_pil[-1]:.3f} s, tree_png / barcode_png {t_dev[-1]:.3f} s", file=sys.stderr, flush=True)
        mp, md = float(np.median(t_pil)), float(np.median(t_dev))
        res["trees_g4"] = dict(pairs=4, files_per_round=n_files, raw_plus_pil_s=t_pil, device_png_s=t_dev, raw_plus_pil_images_per_s=a.n / mp,
                               device_png_images_per_s=a.n / md, speedup=mp / md, rows_and_file_counts_equal=bool(same))
        ok = ok and same
    finally:
        handle.close()
    if a.merge_bench:
        res["bench_py_default_path"] = bench_series(a.merge_bench)
    if not a.quick:
        (REPO / "profiles" / "grid_bench.json").write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
